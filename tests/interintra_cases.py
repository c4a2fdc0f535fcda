"""AV1 inter-intra prediction: reader of tests/golden/interintra.bin (written by tests/golden/gen_golden_interintra.c from the
reference's own C, the prepared edges and the chosen predictors recorded from inside build_intra_predictors) and a numpy
restatement, written from the C, of everything csrc/interintra_plan.h holds: the edge preparation, the DC variants, the
SMOOTH predictor, the smooth masks, the wedge mask of a plane, the blends, and with obmc_pred_cases' single-reference
predictor the whole of svt_aom_inter_prediction with is_interintra_used = 1.  Shared by tests/test_interintra.py (CPU),
tests/test_interintra_plan_header.py and tests/test_interintra_gpu.py."""
import functools
import os

import numpy as np

import golden_io
import masked_compound_cases
import obmc_pred_cases
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interintra.bin")
SIZES = [(8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
PLANE_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)]
KINDS = ("dc", "dc_top", "dc_left", "dc_128", "v", "h", "smooth")  # 7: the early constant fill
MODE_DC, MODE_V, MODE_H, MODE_SMOOTH = range(4)
# sm_weight_arrays (EbIntraPrediction.c:26-45), by block dimension
SM_WEIGHTS = {4: [255, 149, 85, 64], 8: [255, 197, 146, 105, 73, 50, 37, 32],
              16: [255, 225, 196, 170, 145, 123, 102, 84, 68, 54, 43, 33, 26, 20, 17, 16],
              32: [255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111, 101, 92, 83, 74, 66, 59, 52, 45, 39, 34, 29, 25, 21, 17,
                   14, 12, 10, 9, 8, 8]}
# ii_weights1d (EbInterPrediction.c:2137-2145)
II_WEIGHTS = [60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22,
              21, 20, 19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7,
              7, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 4, 4, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,
              2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
COUNTS = dict(size8=(0, 7), size10=(7, 7), mode=(14, 4), wedge=(18, 2), wedge_index=(20, 16), avail=(36, 9), hang=(45, 2), col0=(47, 1),
              row0=(48, 1), right=(49, 1), bottom=(50, 1), form=(51, 4), content=(55, 3), lo=(58, 1), hi=(59, 1), dc_up=(60, 1),
              dc_down=(61, 1), nochroma=(62, 1), chroma=(63, 1), kind=(64, 8))


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


# ---- the rules ----
def prepare_edges(above, left, n_top, n_left, w, h, bd):
    """build_intra_predictors' above_row[w] and left_col[h] for DC, V, H and SMOOTH from the raw neighbour samples."""
    base = 128 << (bd - 8)
    if n_top > 0:
        a = np.concatenate([above[:n_top], np.full(w - n_top, above[n_top - 1])]).astype(np.int64)
    else:
        a = np.full(w, int(left[0]) if n_left > 0 else base - 1, np.int64)
    if n_left > 0:
        l = np.concatenate([left[:n_left], np.full(h - n_left, left[n_left - 1])]).astype(np.int64)
    else:
        l = np.full(h, int(above[0]) if n_top > 0 else base + 1, np.int64)
    return a, l


def kind_of(mode, n_top, n_left):
    """Which predictor build_intra_predictors runs (an index into KINDS), or 7 for its early constant fill."""
    if mode == MODE_V:
        return 4 if n_top > 0 else 7
    if mode == MODE_H:
        return 5 if n_left > 0 else 7
    if mode == MODE_SMOOTH:
        return 6
    return {(1, 1): 0, (1, 0): 1, (0, 1): 2, (0, 0): 3}[(int(n_top > 0), int(n_left > 0))]


def intra_by_kind(kind, a, l, bd):
    """The w x h block of predictor KINDS[kind] from prepared edges a[w], l[h] (int64)."""
    w, h = len(a), len(l)
    if kind == 0:
        return np.full((h, w), (int(a.sum() + l.sum()) + ((w + h) >> 1)) // (w + h), np.int64)
    if kind == 1:
        return np.full((h, w), (int(a.sum()) + (w >> 1)) // w, np.int64)
    if kind == 2:
        return np.full((h, w), (int(l.sum()) + (h >> 1)) // h, np.int64)
    if kind == 3:
        return np.full((h, w), 128 << (bd - 8), np.int64)
    if kind == 4:
        return np.tile(a[None, :], (h, 1))
    if kind == 5:
        return np.tile(l[:, None], (1, w))
    wh, ww = np.asarray(SM_WEIGHTS[h], np.int64)[:, None], np.asarray(SM_WEIGHTS[w], np.int64)[None, :]
    return (wh * a[None, :] + (256 - wh) * l[h - 1] + ww * l[:, None] + (256 - ww) * a[w - 1] + 256) >> 9


def intra(mode, above, left, n_top, n_left, w, h, bd):
    """svt_av1_predict_intra_block for interintra_to_intra_mode[mode] on raw edges: (block, kind, prepared above, left)."""
    a, l = prepare_edges(above, left, n_top, n_left, w, h, bd)
    kind = kind_of(mode, n_top, n_left)
    # the early fill is the V / H predictor on the prepared (constant) row / column
    return intra_by_kind(4 if mode == MODE_V else 5 if mode == MODE_H else kind, a, l, bd), kind, a, l


def smooth_mask(mode, w, h):
    """build_smooth_interintra_mask for a w x h plane block."""
    r, c = np.mgrid[0:h, 0:w]
    if mode == MODE_DC:
        return np.full((h, w), 32, np.int64)
    k = r if mode == MODE_V else c if mode == MODE_H else np.minimum(r, c)
    return np.asarray(II_WEIGHTS, np.int64)[k * (128 // max(w, h))]


def wedge_mask_plane(w, h, index, ss):
    """The wedge mask a plane's blend reads: the luma w x h block's, sign 0; chroma the rounded mean of 2x2."""
    m = masked_compound_cases.wedge_mask(w, h, index, 0).astype(np.int64)
    if not ss:
        return m
    return (m[0::2, 0::2] + m[1::2, 0::2] + m[0::2, 1::2] + m[1::2, 1::2] + 2) >> 2


def blend_a64_mask(src0, src1, mask, subw, subh):
    """svt_aom_blend_a64_mask_c: mask [h << subh][w << subw]."""
    m = mask.astype(np.int64)
    if subw and subh:
        m = (m[0::2, 0::2] + m[1::2, 0::2] + m[0::2, 1::2] + m[1::2, 1::2] + 2) >> 2
    elif subw:
        m = (m[:, 0::2] + m[:, 1::2] + 1) >> 1
    elif subh:
        m = (m[0::2, :] + m[1::2, :] + 1) >> 1
    return (m * src0.astype(np.int64) + (64 - m) * src1.astype(np.int64) + 32) >> 6


def edge_plane_offset(w, h, p):
    return 0 if p == 0 else (w + h) if p == 1 else (w + h) + (w + h) // 2


def block_edges(b, edges, p):
    """Raw above[pw], left[ph] of plane p of block b from the edge pool."""
    ss = int(p > 0)
    pw, ph, o = b["w"] >> ss, b["h"] >> ss, b["edge_offset"] + edge_plane_offset(b["w"], b["h"], p)
    return edges[o:o + pw], edges[o + pw:o + pw + ph]


def predict_batch(refs, pad, blocks, edges, bd, w, h, chroma, border=None, fill=0):
    """The three predictor planes of svtgpu_interintra_predict_batch: blocks dicts with x, y, w, h, ref, fx, fy, mv, mode, use_wedge,
    wedge_index, n_top, n_left (pairs), edge_offset."""
    out = [np.full((h >> (p > 0), w >> (p > 0)), fill, dtype=refs[0][0].dtype) for p in range(3)]
    for b in blocks:
        plain = dict(b, above=[], left=[])
        inter = obmc_pred_cases.predict_batch(refs, pad, [plain], bd, w, h, chroma, border)
        for p in range(3 if chroma else 1):
            ss = int(p > 0)
            pw, ph, ox, oy = b["w"] >> ss, b["h"] >> ss, b["x"] >> ss, b["y"] >> ss
            above, left = block_edges(b, edges, p)
            ip = intra(b["mode"], above, left, b["n_top"][ss], b["n_left"][ss], pw, ph, bd)[0]
            m = wedge_mask_plane(b["w"], b["h"], b["wedge_index"], ss) if b["use_wedge"] else smooth_mask(b["mode"], pw, ph)
            cur = inter[p][oy:oy + ph, ox:ox + pw].astype(np.int64)
            out[p][oy:oy + ph, ox:ox + pw] = (m * ip + (64 - m) * cur + 32) >> 6
    return out


def mode_sse(refs, pad, blocks, edges, bd, w, h, src, border=None):
    """svtgpu_interintra_mode_sse_batch: int64 [n_blocks][4]."""
    out = np.zeros((len(blocks), 4), np.int64)
    for i, b in enumerate(blocks):
        for m in range(4):
            p = predict_batch(refs, pad, [dict(b, mode=m, use_wedge=0)], edges, bd, w, h, 0, border)[0]
            d = src[b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]].astype(np.int64) - \
                p[b["y"]:b["y"] + b["h"], b["x"]:b["x"] + b["w"]].astype(np.int64)
            out[i, m] = int((d * d).sum())
    return out


# ---- the records ----
def source_luma(idx, w, h, bd, content):
    maxv = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    if content == 2:
        return np.full((h, w), maxv, dt)
    if content in (1, 3):
        return np.zeros((h, w), dt)
    return draw(0x4949000000300000 + 256 * idx, w * h, maxv + 1).reshape(h, w).astype(dt)


def _blocks(rows):
    out = []
    for v in rows:
        v = [int(k) for k in v]
        out.append(dict(x=v[0], y=v[1], w=v[2], h=v[3], ref=v[4], fx=v[5], fy=v[6], mv=(v[7], v[8]), mode=v[9], use_wedge=v[10],
                        wedge_index=v[11], n_top=(v[12], v[13]), n_left=(v[14], v[15]), edge_offset=v[16], kinds=tuple(v[17:20]),
                        hang=(v[20], v[21])))
    return out


@functools.lru_cache(maxsize=1)
def records():
    g, out = fixture(), []
    for i in range(int(g["nrec"][0])):
        bd, w, h, nr, chroma, border, nb, content, idx = (int(v) for v in g["r%d_par" % i])
        refs = [obmc_pred_cases.reference_picture(bd, w, h, 0x4949000000100000 + 256 * idx + 4 * r, border, content, r) for r in range(nr)]
        out.append(dict(name="r%d" % i, bd=bd, w=w, h=h, n_refs=nr, chroma=chroma, pad=border, content=content, refs=refs, index=idx,
                        blocks=_blocks(g["r%d_blocks" % i]), edges=g["r%d_edges" % i], prep=g["r%d_prep" % i], sse=g["r%d_sse" % i],
                        pred=[g["r%d_pred%d" % (i, p)] for p in range(3 if chroma else 1)], src=source_luma(idx, w, h, bd, content)))
    return out


@functools.lru_cache(maxsize=1)
def blend_cases():
    """The blend records: dicts with hbd, w, h, subw, subh, bd, src0, src1, mask (rebuilt as the generator drew them), out."""
    g, out = fixture(), []
    for k in range(int(g["nblend"][0])):
        hbd, w, h, subw, subh, bd, idx, ext = (int(v) for v in g["b%d_par" % k])
        seed, dt, mw, mh = 0x4949000000400000 + 16 * idx, np.uint16 if hbd else np.uint8, w << subw, h << subh
        if ext:
            a, b = np.full((h, w), (1 << bd) - 1, dt), np.zeros((h, w), dt)
            y, x = np.mgrid[0:mh, 0:mw]
            m = np.where((x ^ y) & 2, 0, 64).astype(np.uint8)
        else:
            a, b = (draw(seed + j, w * h, 1 << bd).reshape(h, w).astype(dt) for j in (0, 1))
            m = draw(seed + 2, mw * mh, 65).reshape(mh, mw).astype(np.uint8)
        out.append(dict(name="b%d" % k, hbd=hbd, w=w, h=h, subw=subw, subh=subh, bd=bd, src0=a, src1=b, mask=m, out=g["b%d_out" % k]))
    return out


@functools.lru_cache(maxsize=1)
def intra_cases():
    """The intra records: dicts with hbd, w, h, kind, bd, above[w], left[h], out."""
    g, out = fixture(), []
    for k in range(int(g["nintra"][0])):
        hbd, w, h, kind, bd, idx = (int(v) for v in g["i%d_par" % k])
        seed, dt = 0x4949000000500000 + 16 * idx, np.uint16 if hbd else np.uint8
        if idx % 5 == 4:
            a, l = np.full(48, (1 << bd) - 1), np.full(48, (1 << bd) - 1)
        else:
            a, l = draw(seed, 48, 1 << bd), draw(seed + 1, 48, 1 << bd)
        if not hbd:
            a, l = a & 255, l & 255
        out.append(dict(name="i%d" % k, hbd=hbd, w=w, h=h, kind=kind, bd=bd, above=a[8:8 + w].astype(dt), left=l[8:8 + h].astype(dt),
                        out=g["i%d_out" % k]))
    return out


def counts():
    c = [int(v) for v in fixture()["counts"]]
    return {k: c[a:a + n] for k, (a, n) in COUNTS.items()}
