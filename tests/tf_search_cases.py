"""The temporal filter's sub-pel motion search: reader of tests/golden/tf_search.bin (written by
tests/golden/gen_golden_tf_search.c from the reference's own C), the generator's drawn pictures rebuilt, and a numpy
restatement of svt_check_position / tf_subpel_search (EbTemporalFiltering.c:1535-1765), the four tf_*_sub_pel_search block
walks, the 64-vs-32 test, the pred_error_32x32_th bypass and derive_tf_32x32_block_split_flag (:240-289, :3087-3261), on
interp_cases.py's convolve and MV clamp.  Shared by tests/test_tf_search.py (CPU) and tests/test_tf_search_gpu.py."""
import functools
import os

import numpy as np

import golden_io
import interp_cases as ic
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf_search.bin")
W, H, AW, AH, PAD, NR, NBLK = 136, 72, 192, 128, 80, 2, 6
RS, RH, HU, HV = W + 2 * PAD, H + 2 * PAD, 736, 608
M32, M64, INT_MAX = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFF
KINDS = ("use64 by the test", "use64 by force64", "split32 0", "split32 1", "split16 0", "split16 1", "16x16 skipped by threshold",
         "moved in the half stage", "moved in the quarter stage", "moved in the eighth stage", "skipped by the early exit",
         "skipped by best == 0", "ties", "clamp left", "clamp right", "clamp top", "clamp bottom")
FIELDS = ("use64", "mv64", "split32", "split16", "mv32", "mv16", "mv8", "bmv16", "err32", "err16")


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


# ---------------------------------------------------------------------------------------------
# the drawn pictures
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def pictures(bd, low8=False):
    """dict(cen, ref, cen8, ref8): the centre's three planes over the aligned area, the references' three padded planes
    (PAD luma samples around the picture), and their 8-bit search planes (the same at 8 bits; >> 2 with low8)."""
    sc, maxv, S = 1 << (bd - 8), (1 << bd) - 1, 0x5453000000000000 + 16 * (bd > 8)
    v, u = np.mgrid[0:HV, 0:HU]
    coarse = np.repeat(np.repeat(draw(S, 92 * (HV >> 3), 128 * sc).reshape(HV >> 3, 92), 8, axis=0), 8, axis=1)
    tex = np.clip((u + v) * sc // 8 + coarse + draw(S + 1, HU * HV, 16 * sc).reshape(HV, HU), 0, maxv)
    dt = np.uint16 if bd > 8 else np.uint8
    cen, ref = [tex[2 * PAD + 16:2 * PAD + 16 + 2 * AH:2, 2 * PAD + 16:2 * PAD + 16 + 2 * AW:2]], [[] for _ in range(NR)]
    for k in (1, 2):
        y, x = np.mgrid[0:AH // 2, 0:AW // 2]
        cen.append(np.clip(draw(S + 8 + k, (AW // 2) * (AH // 2), 64 * sc).reshape(AH // 2, AW // 2) + (2 * x + y) * sc // 4, 0, maxv))
    y, x = np.mgrid[0:RH, 0:RS]
    cx, cy = x // 24, y // 24
    cell = cy * 13 + cx
    flat = (x - PAD >= 40) & (x - PAD < 88) & (y - PAD >= -32) & (y - PAD < 40)
    for r in range(NR):
        d13, d4 = draw(S + 2 + r, 4 * 130, 13), draw(S + 2 + r, 4 * 130, 4)
        dx, dy, amp = d13[0::4][cell] - 6, d13[1::4][cell] - 6, np.array([0, 2, 8, 24])[d4[2::4]][cell] * sc
        exact, good = (cx == 3) & (cy == 3), (cx >= 5) & (cy >= 5)
        dx, dy, amp = np.where(exact, 2, dx), np.where(exact, 2, dy), np.where(exact, 0, amp)
        dx, dy, amp = np.where(good, 2, dx), np.where(good, 0, dy), np.where(good, 2 * sc, amp)
        dx, dy = np.where(flat, 0, dx), np.where(flat, 0, dy)
        noise = draw(S + 4 + r, RS * RH, (2 * amp + 1).reshape(-1)).reshape(RH, RS) - amp
        a = tex[2 * y + 16 + dy, 2 * x + 16 + dx] + np.where(amp > 0, noise, 0)
        ref[r].append(np.clip(np.where(flat, 100 * sc, a), 0, maxv))
        for k in (1, 2):
            yy, xx = np.mgrid[0:RH // 2, 0:RS // 2]
            ref[r].append(np.clip(draw(S + 10 + 2 * r + k, (RS // 2) * (RH // 2), 64 * sc).reshape(RH // 2, RS // 2) +
                                  (2 * (xx - 40) + (yy - 40) + 160) * sc // 4, 0, maxv))
    sh = 2 if low8 else 0
    return dict(cen=[a.astype(dt) for a in cen], ref=[[a.astype(dt) for a in r] for r in ref],
                cen8=[(a >> sh).astype(np.uint8 if low8 else dt) for a in cen],
                ref8=[[(a >> sh).astype(np.uint8 if low8 else dt) for a in r] for r in ref])


# ---------------------------------------------------------------------------------------------
# the records
# ---------------------------------------------------------------------------------------------
def _records(g, pre):
    return {f: g["%s_%s" % (pre, f)] for f in FIELDS}


def _params(par, th32):
    return dict(bd=par[0], modes=(par[1], par[2], par[3]), use_2tap=par[4], shift=par[5], enable8=par[6], early=par[7], th32=th32)


def _fullpel(g, bd):
    return {k: g["f%d_%s" % (bd, k)] for k in ("mv64", "mv32", "mv16", "mv8")}


@functools.lru_cache(maxsize=1)
def search_cases():
    g = fixture()
    out = []
    for k in range(int(g["nset"][0])):
        par = [int(v) for v in g["s%d_par" % k]]
        out.append(dict(name="s%d_%dbit_set%d" % (k, par[0], par[10]), P=_params(par, int(g["s%d_th32" % k][0])), n_refs=par[8],
                        pad=par[9], set=par[10], pic_bd=par[0], low8=False, force64=g["s%d_force64" % k], fullpel=_fullpel(g, par[0]),
                        want=_records(g, "s%d" % k), kinds=[int(v) for v in g["s%d_kinds" % k]]))
    return out


@functools.lru_cache(maxsize=1)
def chain_cases():
    g = fixture()
    out = []
    for i in range(int(g["nchain"][0])):
        bd, sbd, st, mv_dist_th, chroma, idx = (int(v) for v in g["c%d_par" % i])
        P = dict(search_cases()[st]["P"], bd=sbd)
        out.append(dict(name="c%d_%dbit" % (i, bd), P=P, n_refs=NR, pad=PAD, pic_bd=bd, low8=bd > 8, force64=np.zeros((NR, NBLK), np.uint8),
                        fullpel=_fullpel(g, 10 if bd > 8 else 8), want=_records(g, "c%d" % i), err32p=g["c%d_err32p" % i],
                        mv_dist_th=mv_dist_th, tf_chroma=chroma, decay=[int(v) for v in g["c%d_decay" % i]],
                        pred=[[g["c%d_pred%d_%d" % (i, r, p)] for p in range(3)] for r in range(NR)],
                        out=[g["c%d_out%d" % (i, p)] for p in range(3)]))
    return out


def reachable(c, k):
    """Whether the parameters of search case c can reach count k (the generator's rule)."""
    P = c["P"]
    if k == 1:
        return c["set"] == 8
    if k == 5:
        return bool(P["enable8"])
    if k == 6:
        return P["th32"] != 0
    if 7 <= k <= 9:
        return P["modes"][k - 7] != 0
    if k == 10:
        return P["early"] != 0
    return True


def motion_block_arrays(rec):
    """What the device's records must hold, from records in the fixture's layout: (motion fields, block fields) as dicts of
    arrays [n_refs][nblk][...].  The motion record's mv32 of a use64 block is 0 (the fixture's mv32 there is the block
    record's, = mv64); the block record's mv16 is bmv16."""
    u = rec["use64"].astype(bool)
    mo = dict(use64=rec["use64"], mv64=rec["mv64"], split32=rec["split32"], split16=rec["split16"],
              mv32=np.where(u[..., None, None], 0, rec["mv32"]), mv16=rec["mv16"], mv8=rec["mv8"])
    bl = dict(split32=rec["split32"], mv32=rec["mv32"], mv16=rec["bmv16"], err32=rec["err32"], err16=rec["err16"])
    return mo, bl


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def _i32(v):
    return ((int(v) + (1 << 31)) & M32) - (1 << 31)


def subpel_search(ref, pad, cen, w, h, bd, px, py, b, start, kind, P, border=None, y_outer=False, trace=None):
    """tf_subpel_search of the b x b block at (px, py): ref the padded luma plane, cen the centre's, start the full-pel MV;
    kind the filter table.  Returns (error, mv_x, mv_y).  Test-only switches: y_outer walks the positions of a stage with y
    outer and x inner (not the reference's order); trace, a list, receives one dict per evaluated position (block size,
    MV, convolve form, sse, sum, distortion, and with P["trace_clip"] whether the convolve's final clip changed a sample)."""
    t, shift, hbd = ic.tables(), P["shift"], int(bd > 8)
    n, thr = b * (b >> shift), ((b * b * P["early"]) << hbd) & M32
    c = cen[py:py + b:1 << shift, px:px + b].astype(np.int64)

    def dist(mvx, mvy):
        sx, phx = ic.clamp_mv(mvx, px, b, w, 0)
        sy, phy = ic.clamp_mv(mvy, py, b, h, 0)
        xs, ys = np.arange(sx - 3, sx + b + 4), np.arange(sy - 3, sy + b + 4)
        if border is not None:
            xs, ys = np.clip(xs, -border[0], w + border[0] - 1), np.clip(ys, -border[1], h + border[1] - 1)
        assert xs.min() >= -pad and ys.min() >= -pad and xs.max() < w + pad and ys.max() < h + pad
        form = (1 if phx else 0) | (2 if phy else 0)
        pr = ic.convolve(ref[np.ix_(ys + pad, xs + pad)], b, b, t[kind][phx], t[kind][phy], form, bd)
        d = pr[::1 << shift] - c
        sse, sm = int((d * d).sum()), int(d.sum())
        if trace is not None:
            trace.append(dict(b=b, px=px, py=py, mv=(mvx, mvy), form=form, sse=sse, sum=sm))
            if P.get("trace_clip"):
                raw = ic.convolve(ref[np.ix_(ys + pad, xs + pad)], b, b, t[kind][phx], t[kind][phy], form, bd, clip=False)
                trace[-1]["clipped"] = bool((raw != pr).any())
        if not hbd:
            v = (sse - (((sm * sm) // n) & M32)) & M32
        else:
            m = (sm + 2) >> 2
            v = max((((sse + 8) >> 4) & M32) - (m * m) // n, 0)
        if trace is not None:
            trace[-1]["dist"] = (v << shift) & M32
        return (v << shift) & M32

    best, bx, by = INT_MAX, _i16(start[0] * 8), _i16(start[1] * 8)
    for stage in range(-1, 3):
        md, step, cx, cy = (1, 0, bx, by) if stage < 0 else (P["modes"][stage], 4 >> stage, bx, by)
        if not md:
            continue
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                if (i or j) if stage < 0 else not (i or j):
                    continue
                if (md >= 2 and i and j) or best == 0 or (P["early"] and best < thr):
                    continue
                mx, my = (_i16(cx + j * step), _i16(cy + i * step)) if y_outer else (_i16(cx + i * step), _i16(cy + j * step))
                d = dist(mx, my)
                if d < best:
                    best, bx, by = d, mx, my
    return best, bx, by


def case_pictures(c):
    """The pictures of case c: its own (a `pics` entry, as pictures() lays them out) or the drawn ones."""
    return c["pics"] if "pics" in c else pictures(c["pic_bd"], c["low8"])


def search_frame(c, border=None, refs=None, y_outer=False, trace=None):
    """The whole walk for case c (a search or chain case): records in the fixture's layout.  refs: other padded luma planes
    than the case's own (the read-clamp test).  y_outer / trace: subpel_search's test-only switches."""
    P, pics = c["P"], case_pictures(c)
    cen = pics["cen8"][0]
    rec = dict(use64=np.zeros((NR, NBLK), np.uint8), mv64=np.zeros((NR, NBLK, 2), np.int16), split32=np.zeros((NR, NBLK, 4), np.uint8),
               split16=np.zeros((NR, NBLK, 16), np.uint8), mv32=np.zeros((NR, NBLK, 4, 2), np.int16),
               mv16=np.zeros((NR, NBLK, 16, 2), np.int16), mv8=np.zeros((NR, NBLK, 64, 2), np.int16),
               bmv16=np.zeros((NR, NBLK, 16, 2), np.int16), err32=np.zeros((NR, NBLK, 4), np.uint64),
               err16=np.zeros((NR, NBLK, 16), np.uint64))
    k64 = ic.BILINEAR if P["use_2tap"] else ic.REGULAR
    fp = c["fullpel"]
    for r in range(c["n_refs"]):
        ref = pics["ref8"][r][0] if refs is None else refs[r]

        def go(px, py, b, start, kind):
            return subpel_search(ref, c["pad"], cen, W, H, P["bd"], px, py, b, start, kind, P, border, y_outer, trace)
        for blk in range(NBLK):
            bx, by = (blk % 3) * 64, (blk // 3) * 64
            e64, mx, my = go(bx, by, 64, fp["mv64"][r][blk], k64)
            use64 = bool(c["force64"][r][blk])
            res32 = []
            if not use64:
                res32 = [go(bx + (i & 1) * 32, by + (i >> 1) * 32, 32, fp["mv32"][r][blk][i], k64) for i in range(4)]
                use64 = e64 * 14 < sum(e for e, _, _ in res32) * 16 and e64 < (1 << 18)
            if use64:
                rec["use64"][r, blk], rec["mv64"][r, blk], rec["mv32"][r, blk] = 1, (mx, my), (mx, my)
                continue
            for i in range(4):
                x32, y32, (e32, m32x, m32y) = bx + (i & 1) * 32, by + (i >> 1) * 32, res32[i]
                split32, s16, e16, m16, m8 = 0, [0] * 4, [0] * 4, [None] * 4, [None] * 16
                if not e32 < P["th32"]:
                    tot = 0
                    for j in range(4):
                        x16, y16 = x32 + (j & 1) * 16, y32 + (j >> 1) * 16
                        e, ax, ay = go(x16, y16, 16, fp["mv16"][r][blk][4 * i + j], ic.REGULAR)
                        m16[j], e = (ax, ay), _i32(e)
                        if P["enable8"]:
                            e8 = 0
                            for k in range(4):
                                ek, kx, ky = go(x16 + (k & 1) * 8, y16 + (k >> 1) * 8, 8, fp["mv8"][r][blk][16 * i + 4 * j + k], ic.REGULAR)
                                m8[4 * j + k], e8 = (kx, ky), _i32(e8 + _i32(ek))
                            if not _i32(e * 8) < _i32(e8 * 16):
                                s16[j], e = 1, e8
                        e16[j], tot = e, _i32(tot + e)
                    split32 = int(not _i32(_i32(e32) * 14) < _i32(tot * 16))
                rec["split32"][r, blk, i] = split32
                if not split32:
                    rec["mv32"][r, blk, i], rec["err32"][r, blk, i] = (m32x, m32y), e32
                    continue
                for j in range(4):
                    q = 4 * i + j
                    rec["split16"][r, blk, q], rec["bmv16"][r, blk, q], rec["err16"][r, blk, q] = s16[j], m16[j], e16[j] & M64
                    if s16[j]:
                        rec["mv8"][r, blk, 4 * q:4 * q + 4] = m8[4 * j:4 * j + 4]
                    else:
                        rec["mv16"][r, blk, q] = m16[j]
    return rec


def err32_of_use64(rec, pred_luma, cen_luma, bd, shift):
    """convert_64x64_info_to_32x32_info: err32 of the use64 blocks from the final predictor pictures [n_refs] against the
    centre; the other blocks keep the search's."""
    out = rec["err32"].copy()
    n = 32 * (32 >> shift)
    for r in range(rec["use64"].shape[0]):
        for blk in range(NBLK):
            if not rec["use64"][r, blk]:
                continue
            for i in range(4):
                x, y = (blk % 3) * 64 + (i & 1) * 32, (blk // 3) * 64 + (i >> 1) * 32
                d = pred_luma[r][y:y + 32:1 << shift, x:x + 32].astype(np.int64) - cen_luma[y:y + 32:1 << shift, x:x + 32].astype(np.int64)
                sse, sm = int((d * d).sum()), int(d.sum())
                if bd == 8:
                    v = (sse - (((sm * sm) // n) & M32)) & M32
                else:
                    m = (sm + 2) >> 2
                    v = max((((sse + 8) >> 4) & M32) - (m * m) // n, 0)
                out[r, blk, i] = (v << shift) & M32
    return out


def motion_dicts(rec):
    """The records as interp_cases.predict_frame reads them: [reference][block] dicts."""
    return [[dict(use64=int(rec["use64"][r][b]), mv64=rec["mv64"][r][b], split32=rec["split32"][r][b], split16=rec["split16"][r][b],
                  mv32=rec["mv32"][r][b], mv16=rec["mv16"][r][b], mv8=rec["mv8"][r][b]) for b in range(NBLK)]
            for r in range(rec["use64"].shape[0])]
