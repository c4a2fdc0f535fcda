"""AV1 OBMC prediction: reader of tests/golden/obmc_pred.bin (written by tests/golden/gen_golden_obmc_pred.c from the
reference's own C, the neighbour lists recorded from its own walk) and a numpy restatement, written from the C, of
svt_aom_inter_prediction with motion_mode = OBMC_CAUSAL (EbEncInterPrediction.c:4070, :4507): the block's own
single-reference prediction, the neighbour strips of build_prediction_by_{above,left}_pred (:1144-1343) with the edges of
av1_setup_build_prediction_by_{above,left}_pred (:754-788) and build_prediction_by_{above,left}_preds (:1344-1428), and the
blends of build_obmc_inter_pred_{above,left} (:1441-1535).  Shared by tests/test_obmc_pred.py (CPU) and
tests/test_obmc_pred_gpu.py."""
import functools
import os

import numpy as np

import golden_io
from interp_cases import _i16, convolve, filter_table, tables
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obmc_pred.bin")
SIZES = [(8, 8), (8, 16), (16, 8), (8, 32), (32, 8), (16, 16), (16, 32), (32, 16), (16, 64), (64, 16), (32, 32), (32, 64),
         (64, 32), (64, 64), (64, 128), (128, 64), (128, 128)]
MASKS = {1: [64], 2: [45, 64], 4: [39, 50, 59, 64], 8: [36, 42, 48, 53, 57, 61, 64, 64],
         16: [34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64],
         32: [33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64,
              64, 64]}
MAX_NEIGHBOURS = {8: 1, 16: 2, 32: 3, 64: 4, 128: 4}
PAD = 160  # what content 4 is drawn over
# the fixture's counters (gen_golden_obmc_pred.c's enum)
COUNTS = dict(size8=(0, 17), size10=(17, 17), size10_chroma=(34, 17), size_nochroma=(51, 17), fx=(68, 4), fy=(72, 4), n_above=(76, 5),
              n_left=(81, 5), stopped=(86, 1), gap=(87, 1), wider=(88, 1), pair4=(89, 1), row0=(90, 1), col0=(91, 1), right=(92, 1),
              bottom=(93, 1), mismatch=(94, 4), tap4=(98, 4), compound_nb=(102, 1), lo=(103, 1), hi=(104, 1), ws_zero=(105, 1),
              ws_max=(106, 1), ws_neg=(107, 1))


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


def pred_depth(side, ss):
    return min(max(side >> (ss + 1), 4), 64 >> (ss + 1))


def blend_depth(side, ss):
    return (min(side, 64) >> 1) >> ss


def skip_plane(w, h, ss, direction):
    return direction == 0 and ((w >> ss), (h >> ss)) in ((4, 4), (8, 4), (4, 8))


def clamp_mv_ex(mv, org, extent, spel_size, dim, ss):
    """clamp_mv_to_umv_border_sb with the edges (org, extent: luma) and the spel size (plane samples) apart -> 1/16 sample."""
    sc = 1 - ss
    q = _i16(mv * (1 << sc))
    spel = (4 + spel_size) << 4
    lo = -(org * 8) * (1 << sc) - spel
    hi = ((dim - extent - org) * 8) * (1 << sc) + spel - 16
    return _i16(min(max(q, lo), hi))


def _region(ref, pad, p, border, pw, ph, x0, y0, rw, rh, qx, qy, fxt, fyt, bd):
    """rw x rh samples of plane p of a padded reference at plane position (x0, y0) displaced by (qx, qy) 1/16 sample."""
    t = tables()
    ss = int(p > 0)
    pd = pad >> ss
    phx, phy = qx & 15, qy & 15
    xs, ys = np.arange(x0 + (qx >> 4) - 3, x0 + (qx >> 4) + rw + 4), np.arange(y0 + (qy >> 4) - 3, y0 + (qy >> 4) + rh + 4)
    if border is not None:
        xs = np.clip(xs, -(border[0] >> ss), pw + (border[0] >> ss) - 1)
        ys = np.clip(ys, -(border[1] >> ss), ph + (border[1] >> ss) - 1)
    form = (1 if phx else 0) | (2 if phy else 0)
    if not form & 1:
        xs[:3], xs[-4:] = xs[3], xs[-5]
    if not form & 2:
        ys[:3], ys[-4:] = ys[3], ys[-5]
    assert xs.min() >= -pd and ys.min() >= -pd and xs.max() < pw + pd and ys.max() < ph + pd
    win = ref[p][np.ix_(ys + pd, xs + pd)]
    return convolve(win, rw, rh, t[fxt][phx], t[fyt][phy], form, bd)


def predict_batch(refs, pad, blocks, bd, w, h, chroma, border=None, fill=0, plain_clamp=False):
    """refs: per reference three padded planes; blocks: dicts with x, y, w, h, ref, fx, fy, mv, above, left (lists of dicts
    rel, size, ref, fx, fy, mv).  Returns the three predictor planes.  plain_clamp (tests only): the strips' across clamp with
    spel from extent >> ss, which the reference does not do."""
    out = [np.full((h >> (p > 0), w >> (p > 0)), fill, dtype=refs[0][0].dtype) for p in range(3)]
    for b in blocks:
        for p in range(3 if chroma else 1):
            ss = int(p > 0)
            bw, bh, pw, ph = b["w"] >> ss, b["h"] >> ss, w >> ss, h >> ss
            ox, oy = b["x"] >> ss, b["y"] >> ss
            qx = clamp_mv_ex(b["mv"][0], b["x"], b["w"], bw, w, ss)
            qy = clamp_mv_ex(b["mv"][1], b["y"], b["h"], bh, h, ss)
            cur = _region(refs[b["ref"]], pad, p, border, pw, ph, ox, oy, bw, bh, qx, qy, filter_table(b["fx"], bw),
                          filter_table(b["fy"], bh), bd).astype(np.int64)
            for direction, spans in ((0, b["above"]), (1, b["left"])):
                if skip_plane(b["w"], b["h"], ss, direction):
                    continue
                side, side_dim, side_org = (b["h"], h, b["y"]) if direction == 0 else (b["w"], w, b["x"])
                al_dim, al_org = (w, b["x"]) if direction == 0 else (h, b["y"])
                pdep, bdep, ext = pred_depth(side, ss), blend_depth(side, ss), min(side // 2, 32)
                m = np.asarray(MASKS[bdep], dtype=np.int64)
                for n in spans:
                    along, a0 = (4 * n["size"]) >> ss, (4 * n["rel"]) >> ss
                    q_al = clamp_mv_ex(n["mv"][direction], al_org + 4 * n["rel"], 4 * n["size"], along, al_dim, ss)
                    q_ac = clamp_mv_ex(n["mv"][1 - direction], side_org, ext, (ext >> ss) if plain_clamp else pdep, side_dim, ss)
                    if direction == 0:
                        strip = _region(refs[n["ref"]], pad, p, border, pw, ph, ox + a0, oy, along, pdep, q_al, q_ac,
                                        filter_table(n["fx"], along), filter_table(n["fy"], pdep), bd)
                        a = cur[:bdep, a0:a0 + along]
                        cur[:bdep, a0:a0 + along] = (m[:, None] * a + (64 - m[:, None]) * strip[:bdep] + 32) >> 6
                    else:
                        strip = _region(refs[n["ref"]], pad, p, border, pw, ph, ox, oy + a0, pdep, along, q_ac, q_al,
                                        filter_table(n["fx"], pdep), filter_table(n["fy"], along), bd)
                        a = cur[a0:a0 + along, :bdep]
                        cur[a0:a0 + along, :bdep] = (m[None, :] * a + (64 - m[None, :]) * strip[:, :bdep] + 32) >> 6
            out[p][oy:oy + bh, ox:ox + bw] = cur
    return out


def weighted_src(refs, pad, b, src, w, h, border=None):
    """(wsrc, mask) of block b, int64 [h][w] each: calc_target_weighted_pred (EbEncInterPrediction.c:1767-1827) on the 8-bit
    luma strips of the block's spans; src the source luma picture."""
    bw, bh = b["w"], b["h"]
    ws, mk = np.zeros((bh, bw), np.int64), np.full((bh, bw), 64, np.int64)
    for direction, spans in ((0, b["above"]), (1, b["left"])):
        side, side_dim, side_org = (bh, h, b["y"]) if direction == 0 else (bw, w, b["x"])
        al_dim, al_org = (w, b["x"]) if direction == 0 else (h, b["y"])
        dep, ext = blend_depth(side, 0), min(side // 2, 32)
        m = np.asarray(MASKS[dep], dtype=np.int64)
        for n in spans:
            along, a0 = 4 * n["size"], 4 * n["rel"]
            q_al = clamp_mv_ex(n["mv"][direction], al_org + a0, along, along, al_dim, 0)
            q_ac = clamp_mv_ex(n["mv"][1 - direction], side_org, ext, pred_depth(side, 0), side_dim, 0)
            if direction == 0:
                p = _region(refs[n["ref"]], pad, 0, border, w, h, b["x"] + a0, b["y"], along, dep, q_al, q_ac,
                            filter_table(n["fx"], along), filter_table(n["fy"], dep), 8)
                ws[:dep, a0:a0 + along], mk[:dep, a0:a0 + along] = (64 - m[:, None]) * p, m[:, None]
            else:
                p = _region(refs[n["ref"]], pad, 0, border, w, h, b["x"], b["y"] + a0, dep, along, q_ac, q_al,
                            filter_table(n["fx"], dep), filter_table(n["fy"], along), 8)
                ws[a0:a0 + along, :dep] = (ws[a0:a0 + along, :dep] >> 6) * m[None, :] + (p << 6) * (64 - m[None, :])
                mk[a0:a0 + along, :dep] = (mk[a0:a0 + along, :dep] >> 6) * m[None, :]
        if direction == 0:
            ws, mk = ws * 64, mk * 64
    return src[b["y"]:b["y"] + bh, b["x"]:b["x"] + bw].astype(np.int64) * 4096 - ws, mk


def source_luma(idx, w, h, content):
    """The source luma picture of record idx (gen_golden_obmc_pred.c: gen_record)."""
    if content == 2:
        return np.full((h, w), 255, np.uint8)
    if content in (1, 3):
        return np.zeros((h, w), np.uint8)
    return draw(0x4F42000000200000 + 256 * idx, w * h, 256).reshape(h, w).astype(np.uint8)


@functools.lru_cache(maxsize=1)
def blend_cases():
    """The six blend functions' records: dicts with fn (0 vmask, 1 hmask, 2 / 3 the _16bit forms, 4 / 5 the _8bit forms), w, h,
    bd, src0, src1, mask (rebuilt as the generator drew them) and out."""
    g, out = fixture(), []
    for k in range(int(g["nblend"][0])):
        fn, w, h, bd, idx, ext = (int(v) for v in g["m%d_par" % k])
        seed, dt = 0x4F42000000300000 + 16 * idx, np.uint8 if fn < 2 else np.uint16
        if ext:
            a, b = np.full((h, w), (1 << bd) - 1, dt), np.zeros((h, w), dt)
            m = np.where(np.arange(128) & 1, 0, 64)
        else:
            a, b = (draw(seed + j, w * h, 1 << bd).reshape(h, w).astype(dt) for j in (0, 1))
            m = draw(seed + 2, 128, 65)
        out.append(dict(name="m%d" % k, fn=fn, w=w, h=h, bd=bd, src0=a, src1=b, mask=[int(v) for v in m[:w if fn & 1 else h]],
                        out=g["m%d_out" % k]))
    return out


def blend(c):
    m = np.asarray(c["mask"], np.int64)
    m = m[None, :] if c["fn"] & 1 else m[:, None]
    return (m * c["src0"].astype(np.int64) + (64 - m) * c["src1"].astype(np.int64) + 32) >> 6


def _draw_at(seed, idx, mod):
    """Samples idx[] of the generator's stream `seed` (tf_cases.draw for arbitrary indices)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(mod)).astype(np.int64)


def reference_picture(bd, w, h, seed, pad, content, r):
    """The three padded planes of reference r of a record (gen_golden_obmc_pred.c: pic_value, ref_alloc)."""
    sc, maxv, planes = 1 << (bd - 8), (1 << bd) - 1, []
    dt = np.uint16 if bd > 8 else np.uint8
    for p in range(3):
        pw, ph, pd = w >> (p > 0), h >> (p > 0), pad >> (p > 0)
        y, x = np.mgrid[0:ph, 0:pw]
        if content == 4:
            yy, xx = np.mgrid[-pd:ph + pd, -pd:pw + pd]
            idx = ((yy + PAD) * 4096 + xx + 2048).astype(np.uint64).ravel()
            planes.append(_draw_at(seed + p, idx, maxv + 1).reshape(yy.shape).astype(dt))
            continue
        if content == 0:
            a = np.clip((2 * x + y) * sc // 4 + draw(seed + p, pw * ph, 64 * sc).reshape(ph, pw), 0, maxv)
        elif content in (1, 2):
            a = np.full((ph, pw), 0 if content == 1 else maxv, dtype=np.int64)
        else:
            a = np.where((x + y + r) & 1, maxv, 0)
        planes.append(np.pad(a, pd, mode="edge").astype(dt))
    return planes


def _blocks(rows):
    out = []
    for v in rows:
        v = [int(k) for k in v]
        nb = [dict(rel=v[11 + 7 * k], size=v[12 + 7 * k], ref=v[13 + 7 * k], fx=v[14 + 7 * k], fy=v[15 + 7 * k],
                   mv=(v[16 + 7 * k], v[17 + 7 * k])) for k in range(8)]
        out.append(dict(x=v[0], y=v[1], w=v[2], h=v[3], ref=v[4], fx=v[5], fy=v[6], mv=(v[7], v[8]), above=nb[:v[9]],
                        left=nb[4:4 + v[10]]))
    return out


@functools.lru_cache(maxsize=1)
def records():
    g = fixture()
    out = []
    for i in range(int(g["nrec"][0])):
        bd, w, h, nr, chroma, border, nb, content, idx = (int(v) for v in g["r%d_par" % i])
        refs = [reference_picture(bd, w, h, 0x4F42000000100000 + 256 * idx + 4 * r, border, content, r) for r in range(nr)]
        out.append(dict(name="r%d" % i, bd=bd, w=w, h=h, n_refs=nr, chroma=chroma, pad=border, content=content, refs=refs,
                        blocks=_blocks(g["r%d_blocks" % i]), pred=[g["r%d_pred%d" % (i, p)] for p in range(3 if chroma else 1)], index=idx,
                        wm=[(int(j), g["r%d_wsrc%d" % (i, k)], g["r%d_wmask%d" % (i, k)]) for k, j in enumerate(g["r%d_wmidx" % i])]))
    return out


def counts():
    c = [int(v) for v in fixture()["counts"]]
    return {k: c[a:a + n] for k, (a, n) in COUNTS.items()}
