"""The temporal filter on worst-case and all-tie content: reader of tests/golden/tf_extreme.bin (written by
tests/golden/gen_golden_tf_search.c --extreme from the reference's own C) and the generator's planes rebuilt from their
formulas.  The cases carry their own pictures (a `pics` entry) through tf_search_cases.search_frame, err32_of_use64,
interp_cases.predict_frame and tf_cases.filter_frame.  Shared by tests/test_tf_extreme.py (CPU) and
tests/test_tf_extreme_gpu.py."""
import functools
import os

import numpy as np

import golden_io
import tf_search_cases as tc
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf_extreme.bin")
CLASSES = ("max_zero", "inv_checker_pinned", "inv_checker_walk", "flat_ref", "v_stripes", "h_stripes", "th32_wide", "near_max")
MAX_ZERO, CHECKER, FLAT, VSTRIPE, HSTRIPE, CHECKER2, NEAR_MAX = range(7)  # the contents (par[11]); CHECKER2 has cells of 2 x 2
FILTERS = ("wide_frame", "refs26_8bit", "refs26_10bit")
DECAY = (6000000, 9000000, 12000000)


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


def _value(kind, r, x, y, maxv, sc):
    """Sample (x, y) of a plane in the picture's coordinates of that plane; r < 0: the centre."""
    if kind == MAX_ZERO:
        return np.full(x.shape, 0 if r == 0 else maxv, np.int64)
    if kind == CHECKER:
        return np.where(((x + y) & 1) == (r < 0), maxv, 0)
    if kind == FLAT:
        return np.full(x.shape, 100 * sc, np.int64)
    if kind == NEAR_MAX:
        return maxv - (x & 1) if r < 0 else np.zeros(x.shape, np.int64)
    if kind == CHECKER2:
        return np.where(((((x + 800) >> 1) + ((y + 800) >> 1)) & 1) == (r < 0), maxv, 0)
    u = x if kind == VSTRIPE else y
    return np.where(((u + (0 if r < 0 else 3) + 800) >> 2) & 1, maxv, 0)


@functools.lru_cache(maxsize=None)
def pictures(bd, kind):
    """The planes of content `kind` as tf_search_cases.pictures lays them out (the search planes are the pictures')."""
    sc, maxv, dt = 1 << (bd - 8), (1 << bd) - 1, np.uint16 if bd > 8 else np.uint8
    cen, ref = [], [[] for _ in range(tc.NR)]
    for k in range(3):
        ss = int(k > 0)
        y, x = np.mgrid[0:tc.AH >> ss, 0:tc.AW >> ss]
        cen.append(tc.pictures(bd)["cen"][k] if kind == FLAT else _value(kind, -1, x, y, maxv, sc).astype(dt))
        y, x = np.mgrid[0:tc.RH >> ss, 0:tc.RS >> ss]
        for r in range(tc.NR):
            ref[r].append(_value(kind, r, x - (tc.PAD >> ss), y - (tc.PAD >> ss), maxv, sc).astype(dt))
    return dict(cen=cen, ref=ref, cen8=cen, ref8=ref)


@functools.lru_cache(maxsize=None)
def fullpel(kind):
    """The full-pel MVs: 0, but flat_ref's, which the walk must leave as they are."""
    out = {}
    for lvl, name in enumerate(("mv64", "mv32", "mv16", "mv8")):
        n = 1 << (2 * lvl)
        a = np.zeros((tc.NR, tc.NBLK, n, 2), np.int16)
        if kind == FLAT:
            r, b, i = np.mgrid[0:tc.NR, 0:tc.NBLK, 0:n]
            a[..., 0], a[..., 1] = (i + b + r) % 5 - 2, (i + 2 * b + lvl) % 3 - 1
        out[name] = a[:, :, 0] if lvl == 0 else a
    return out


@functools.lru_cache(maxsize=1)
def search_cases():
    g = fixture()
    out = []
    for k in range(int(g["nset"][0])):
        par = [int(v) for v in g["s%d_par" % k]]
        P = tc._params(par, int(g["s%d_th32" % k][0]))
        name = "s%d_%s_%dbit_m%d_t%d_s%d_e%d" % (k, CLASSES[par[10]], par[0], par[1], par[4], par[5], par[6])
        out.append(dict(name=name, P=P, n_refs=par[8], pad=par[9], cls=CLASSES[par[10]], kind=par[11], pic_bd=par[0], low8=False,
                        force64=g["s%d_force64" % k], fullpel=fullpel(par[11]), pics=pictures(par[0], par[11]),
                        want=tc._records(g, "s%d" % k), kinds=[int(v) for v in g["s%d_kinds" % k]]))
    return out


@functools.lru_cache(maxsize=1)
def chain_cases():
    g = fixture()
    out = []
    for i in range(int(g["nchain"][0])):
        bd, sbd, st, mv_dist_th, chroma, _ = (int(v) for v in g["c%d_par" % i])
        s = search_cases()[st]
        out.append(dict(s, name="c%d_%s_%dbit" % (i, s["cls"], bd), P=dict(s["P"], bd=sbd), force64=g["c%d_force64" % i],
                        want=tc._records(g, "c%d" % i), err32p=g["c%d_err32p" % i], mv_dist_th=mv_dist_th, tf_chroma=chroma,
                        decay=[int(v) for v in g["c%d_decay" % i]],
                        pred=[[g["c%d_pred%d_%d" % (i, r, p)] for p in range(3)] for r in range(tc.NR)],
                        out=[g["c%d_out%d" % (i, p)] for p in range(3)]))
    return out


def block_metas(rec, err32):
    """tf_cases.filter_frame's metadata [reference][block] from search records and the patched err32."""
    _, bl = tc.motion_block_arrays(rec)
    return [[dict(split=bl["split32"][r][b].astype(np.int32), mv32=bl["mv32"][r][b], mv16=bl["mv16"][r][b], err32=err32[r][b],
                  err16=bl["err16"][r][b]) for b in range(tc.NBLK)] for r in range(rec["use64"].shape[0])]


@functools.lru_cache(maxsize=1)
def filter_cases():
    """wide_frame and refs26: predictor pictures given directly over the aligned area."""
    g = fixture()
    out = []
    for i in range(int(g["nfilter"][0])):
        bd, w, h, nr, th, _ = (int(v) for v in g["x%d_par" % i])
        aw, ah, maxv, dt = (w + 63) & ~63, (h + 63) & ~63, (1 << bd) - 1, np.uint16 if bd > 8 else np.uint8
        nblk = (aw // 64) * (ah // 64)
        centre, refs = [], [[] for _ in range(nr)]
        for k in range(3):
            y, x = np.mgrid[0:ah >> (k > 0), 0:aw >> (k > 0)]
            v = np.where((x + y) & 1, maxv, 0)
            centre.append(v.astype(dt))
            for r in range(nr):
                if i:  # refs26: even predictors the centre, odd ones its inverse
                    a = maxv - v if r & 1 else v
                else:  # wide_frame: the centre, its inverse, the centre +- 300 of noise
                    a = v if r == 0 else maxv - v if r == 1 else np.clip(v + draw(0x5458000000000000 + k, v.size, 601).reshape(v.shape) - 300, 0, maxv)
                refs[r].append(a.astype(dt))
        m = {f: g["x%d_%s" % (i, f)] for f in ("split", "mv32", "mv16", "err32", "err16")}
        metas = [[{f: v[r][b] for f, v in m.items()} for b in range(nblk)] for r in range(nr)]
        out.append(dict(name=FILTERS[i], bd=bd, w=w, h=h, n_refs=nr, nblk=nblk, mv_dist_th=th, tf_chroma=1, zz=0,
                        decay=[int(v) for v in g["x%d_decay" % i]], centre=centre, refs=refs, metas=metas, wt=g["x%d_wt" % i],
                        wide=g["x%d_wide" % i], occ=g["x%d_occ" % i], out=[g["x%d_out%d" % (i, p)] for p in range(3)]))
    return out
