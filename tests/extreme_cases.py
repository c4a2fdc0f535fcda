"""Worst-case and all-tie contents for the search kernels, with the CPU oracle's answer on each case.

Shared by test_extreme_content.py (CPU: the oracle against a plain numpy / int64 restatement, and the "reach"
assertions that a case really drives a field to the magnitude it is meant to) and test_extreme_content_gpu.py (the
device against the oracle, bit for bit).  Every case is built once (lru_cache) and its arrays are read-only.

Contents, per plane, with maxv = 2^bd - 1: zero, max, checker (0 / maxv by (x + y) & 1), anti (its complement), flat
(100 << (bd - 8)), stripe4 / stripe8 (period 4 / 8 in x and in y), sparse_max (zeros with four isolated maxv samples),
sparse_zero (its complement), tile_max (one 64x64 tile of maxv in a zero plane), tile_zero (its complement), noise
(the synthetic source the rest of the suite uses)."""
import functools

import numpy as np

import oracle
import svtgpu
import synth

CONTENTS = ("zero", "max", "checker", "anti", "flat", "stripe4", "stripe8", "sparse_max", "sparse_zero", "tile_max",
            "tile_zero")
I64_MAX = np.iinfo(np.int64).max


def _dt(bd):
    return np.uint16 if bd > 8 else np.uint8


def plane(name, w, h, bd):
    """One (h, w) plane of the named content."""
    maxv = (1 << bd) - 1
    yy, xx = np.indices((h, w))
    if name in ("zero", "max", "flat"):
        a = np.full((h, w), {"zero": 0, "max": maxv, "flat": 100 << (bd - 8)}[name])
    elif name in ("checker", "anti"):
        a = np.where(((xx + yy) & 1) == (name == "checker"), maxv, 0)
    elif name in ("stripe4", "stripe8"):
        n = int(name[-1])
        a = ((xx % n) ^ (yy % n)) * maxv // (n - 1)
    elif name in ("sparse_max", "sparse_zero"):
        # four isolated samples (one in the last column, one in the last row): few enough that a 64x64 unit's
        # average stays 0 (or maxv - 1 for the complement)
        a = np.zeros((h, w), np.int64)
        for y, x in ((1, 2), (h // 2, w // 2 + 1), (h - 3, w - 1), (h - 1, 5)):
            a[y, x] = maxv
        if name == "sparse_zero":
            a = maxv - a
    elif name in ("tile_max", "tile_zero"):
        a = np.zeros((h, w), np.int64)
        y0, x0 = (64 if h >= 128 else 0), (128 if w >= 192 else 0)  # on the 64-sample tile grid
        a[y0:y0 + 64, x0:x0 + 64] = maxv
        if name == "tile_zero":
            a = maxv - a
    else:
        raise KeyError(name)
    return a.astype(_dt(bd))


def planes(name, w, h, bd, seed=0):
    """[Y, U, V] (4:2:0) of the named content, each plane built at its own size; "noise": the synthetic source."""
    if name == "noise":
        return [np.ascontiguousarray(a) for a in synth.frame_pair(w, h, bd, 0x5EED0E00 + seed + w + 3 * h + bd)[0]]
    return [plane(name, w if p == 0 else w // 2, h if p == 0 else h // 2, bd) for p in range(3)]


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def trunc_div(a, d):
    """C's integer division (towards zero) of an int64 array."""
    return np.sign(a) * (np.abs(a) // d)


# --------------------------------------------------------------------------------------------- 1. Wiener statistics
WINS = (7, 5, 3)
_STATS_PAIRS = (("sparse_max", "max"), ("sparse_zero", "zero"), ("checker", "anti"), ("flat", "flat"))
# (unit w, unit h, bd, dgd content, src content).  64x64: one tile, 1024 px per wave; 70x66: partial last tiles with
# masked columns; 256x256 (10 bit): 16 tiles, the tile partials summed in i64, one whole tile at v = +-960
STATS_CASES = [(w, h, bd, d, s) for (w, h) in ((64, 64), (70, 66)) for bd in (8, 10) for d, s in _STATS_PAIRS] + \
              [(256, 256, 10, "tile_max", "max"), (256, 256, 10, "tile_zero", "zero")]


@functools.lru_cache(maxsize=None)
def stats_case(w, h, bd, dname, sname):
    """(dgd, src): uint16 [h + 8][w + 8] with the unit at (4, 4) and the edge replicated into the border (the layout
    of oracle_compute_stats), and {win: (M, H)} from the oracle."""
    dgd = np.pad(plane(dname, w, h, bd).astype(np.uint16), 4, mode="edge")
    src = np.pad(plane(sname, w, h, bd).astype(np.uint16), 4, mode="edge")
    want = {win: oracle.compute_stats(win, dgd, src, w, h, bd) for win in WINS}
    _freeze(dgd, src, *[a for v in want.values() for a in v])
    return dgd, src, want


def stats_features(win, dgd, src, w, h, rows=None, cols=None):
    """The feature matrix [win^2 + 1][pixels] of svt_av1_compute_stats over the unit (or its rows / cols slice):
    feature k * win + q is dgd[i + q - half][j + k - half] - avg, the last one src[i][j] - avg."""
    half = win >> 1
    avg = int(dgd[4:4 + h, 4:4 + w].astype(np.int64).sum() // (w * h))
    D, X = dgd.astype(np.int64) - avg, src.astype(np.int64) - avg
    rows = slice(0, h) if rows is None else rows
    cols = slice(0, w) if cols is None else cols
    ys, xs = np.arange(h)[rows], np.arange(w)[cols]
    F = [D[np.ix_(4 + ys + q, 4 + xs + k)].ravel() for k in range(-half, half + 1) for q in range(-half, half + 1)]
    F.append(X[np.ix_(4 + ys, 4 + xs)].ravel())
    return np.stack(F)


def stats_numpy(win, dgd, src, w, h, bd):
    """M, H restated: the Gram matrix of the features in float64 (every product is below 2^20 and every sum below
    2^37, so the float sums are exact), each total divided once as C divides."""
    F = stats_features(win, dgd, src, w, h).astype(np.float64)
    G = np.rint(F @ F.T).astype(np.int64)
    n, div = win * win, {8: 1, 10: 4, 12: 16}[bd]
    return trunc_div(G[:n, n], div), trunc_div(G[:n, :n], div).reshape(-1)


def stats_largest_wave_fold(win, dgd, src, w, h):
    """The largest |sum| one wave of wiener_stats_kernel folds into an i32: over every 64x64 tile of the unit, every
    wave (tile rows i = wave mod 4) and every pair of features."""
    best = 0
    for y0 in range(0, h, 64):
        for x0 in range(0, w, 64):
            for wave in range(4):
                F = stats_features(win, dgd, src, w, h, slice(y0 + wave, min(y0 + 64, h), 4),
                                   slice(x0, min(x0 + 64, w))).astype(np.float64)
                best = max(best, int(np.abs(F @ F.T).max()))
    return best


def stats_hi_range(dgd, src, w, h):
    """(min, max) of hi = v >> 5 over every value the kernel stages: the unit's window of dgd - avg and src - avg."""
    avg = int(dgd[4:4 + h, 4:4 + w].astype(np.int64).sum() // (w * h))
    v = np.concatenate([(dgd[1:h + 7, 1:w + 7].astype(np.int64) - avg).ravel(),
                        (src[4:4 + h, 4:4 + w].astype(np.int64) - avg).ravel()])
    return int((v >> 5).min()), int((v >> 5).max())


# --------------------------------------------------------------------------------------------- 2. LR search
LR_UNIT_SIZE = [64, 32, 32]
LR_PAIRS = (("flat", "flat"), ("flat", "noise"), ("checker", "noise"), ("checker", "anti"), ("sparse_max", "zero"),
            ("max", "zero"))
LR_CASES = [(w, h, bd, r, s) for (w, h) in ((136, 72), (128, 128)) for bd in (8, 10) for r, s in LR_PAIRS]
LR_NEED_WIENER = (("checker", "noise"), ("sparse_max", "zero"))  # every plane: >= 1 unit with an evaluated Wiener


def lr_ctrls(mod=oracle):
    return mod.lr_controls(1, 1, rdmult=7000, switchable=(300, 700, 900), wiener=(250, 800), sgrproj=(250, 900))


@functools.lru_cache(maxsize=None)
def lr_case(w, h, bd, rname, sname):
    """(rec, src, frame types, units, records, restored frame) of the oracle's search and apply."""
    rec, src = planes(rname, w, h, bd), planes(sname, w, h, bd)
    ft, units, recs = oracle.lr_search_frame(rec, src, bd, LR_UNIT_SIZE, lr_ctrls())
    out = oracle.lr_apply_frame(rec, rec, bd, ft, LR_UNIT_SIZE, units)
    _freeze(*rec, *src, *units, *recs, *out)
    return rec, src, ft, units, recs, out


# --------------------------------------------------------------------------------------------- 3. MD batch
MD_PAIRS = (("max", "zero"), ("zero", "max"), ("checker", "anti"), ("flat", "flat"))
MD_CASES = [(w, bd, s, r) for w in (64, 72) for bd in (8, 10) for s, r in MD_PAIRS]
MD_NREF = 2
# the origin, one MV reaching past each frame edge (on a 64- or 72-sample frame every non-zero MV does; odd ones
# also flip the checkerboard's phase), and two that put the whole block outside the frame
MD_MVS = ((0, 0), (-5, 0), (7, 0), (0, -6), (0, 9), (-3, 11), (-140, -75), (150, 139))


def md_mv_sets(w):
    """MV arrays [nsb][nref][2] that together give every MD_MVS entry to some (SB, reference)."""
    nsb = ((w + 63) // 64) ** 2
    per, sets = nsb * MD_NREF, []
    for s in range((len(MD_MVS) + per - 1) // per):
        sets.append(np.array([MD_MVS[(s * per + i) % len(MD_MVS)] for i in range(per)], np.int16)
                    .reshape(nsb, MD_NREF, 2))
    return sets


@functools.lru_cache(maxsize=None)
def md_case(w, bd, sname, rname):
    """(src luma, [ref luma] * 2, [(mv, oracle result)])"""
    src, ref = plane(sname, w, w, bd), plane(rname, w, w, bd)
    runs = []
    for mv in md_mv_sets(w):
        want = oracle.md_dist_batch(src, [ref] * MD_NREF, bd, mv)
        _freeze(mv, want)
        runs.append((mv, want))
    _freeze(src, ref)
    return src, [ref] * MD_NREF, runs


def md_numpy(src, ref, bd, mv):
    """uint32 [nsb][nref][3][849] from int64 sums, and the raw (unrounded) SSE of every block."""
    h, w = src.shape
    nsbx = (w + 63) // 64
    nsb = nsbx * ((h + 63) // 64)
    out = np.zeros((nsb, mv.shape[1], 3, oracle.MD_BLOCKS), np.uint32)
    raw = np.zeros((nsb, mv.shape[1], oracle.MD_BLOCKS), np.int64)
    S, R = src.astype(np.int64), ref.astype(np.int64)
    for sb in range(nsb):
        oy, ox = 64 * (sb // nsbx), 64 * (sb % nsbx)
        s = S[np.ix_(np.minimum(oy + np.arange(64), h - 1), np.minimum(ox + np.arange(64), w - 1))]
        for r in range(mv.shape[1]):
            mx, my = int(mv[sb, r, 0]), int(mv[sb, r, 1])
            d = s - R[np.ix_(np.clip(oy + my + np.arange(64), 0, h - 1), np.clip(ox + mx + np.arange(64), 0, w - 1))]
            k = 0
            for bw, bh in oracle.MD_SHAPES:
                blk = lambda a: a.reshape(64 // bh, bh, 64 // bw, bw).sum(axis=(1, 3)).ravel()
                sad, sse, tot = blk(np.abs(d)), blk(d * d), blk(d)
                n = sad.size
                raw[sb, r, k:k + n] = sse
                if bd > 8:  # highbd_10_variance: sse rounded >> 4, sum rounded >> 2, variance clamped at 0
                    sse = (sse + 8) >> 4
                    rs = (tot + 2) >> 2
                    var = np.maximum(sse - rs * rs // (bw * bh), 0)
                else:       # 32-bit sse; variance in uint32
                    var = sse - tot * tot // (bw * bh)
                out[sb, r, 0, k:k + n] = sad
                out[sb, r, 1, k:k + n] = sse & 0xFFFFFFFF
                out[sb, r, 2, k:k + n] = var & 0xFFFFFFFF
                k += n
    return out, raw


# --------------------------------------------------------------------------------------------- 5. ME search
ME_SIZES = ((128, 64), (136, 72))
ME_AREAS = ((13, 37), (45, 11))  # the first crosses a 32-row band with a width that is no multiple of 4
ME_KINDS = ("flat", "max_zero", "stripe4", "stripe8", "beyond", "edge_tie")
ME_CASES = [(w, h, saw, sah, sub, k) for (w, h) in ME_SIZES for (saw, sah) in ME_AREAS for sub in (0, 1)
            for k in ME_KINDS]
ME_NREF = 2


@functools.lru_cache(maxsize=None)
def me_frames(w, h, kind):
    """(src, [ref0, ref1], origin [nsb][2][2]) of one content kind (8-bit luma)."""
    nsb = ((w + 63) // 64) * ((h + 63) // 64)
    org = np.zeros((nsb, ME_NREF, 2), np.int16)
    if kind == "beyond":
        # reference 0: the whole area past the right and the bottom edge (every position reads the corner sample);
        # reference 1: past the bottom edge only (every row reads the last row: ties in y alone, over waves and bands)
        src = planes("noise", w, h, 8, 1)[0]
        refs = [planes("noise", w, h, 8, 2 + r)[0] for r in range(ME_NREF)]
        org[:, 0] = (w + 5, h + 3)
        org[:, 1] = (-9, h + 1)
    elif kind == "edge_tie":
        # one step short of "beyond": reference 0's first search row still reads one real row and reference 1's first
        # column one real column, so where position 0 is not the minimum the tie starts at row (column) 1 -- the
        # first minimum then belongs to wave 1, not to wave 0, whose first tied row is 4
        src = planes("noise", w, h, 8, 1)[0]
        refs = [planes("noise", w, h, 8, 2 + r)[0] for r in range(ME_NREF)]
        nsbx = (w + 63) // 64
        for sb in range(nsb):
            org[sb, 0] = (-9, h - 2 - 64 * (sb // nsbx))
            org[sb, 1] = (w - 2 - 64 * (sb % nsbx), -5)
    else:
        s, r = {"flat": ("flat", "flat"), "max_zero": ("max", "zero"), "stripe4": ("stripe4", "stripe4"),
                "stripe8": ("stripe8", "stripe8")}[kind]
        src, refs = plane(s, w, h, 8), [plane(r, w, h, 8)] * ME_NREF
        # a stripe pattern matches itself only where the whole window lies inside the frame (the clamped border is
        # not periodic): these origins keep shifts 0 and +8 in x (and, on the 72-row frame, in y) inside both areas
        org[:, 0] = (-2, -3)
        org[:, 1] = (-1, -2)
    _freeze(src, org, *refs)
    return src, refs, org


@functools.lru_cache(maxsize=None)
def me_case(w, h, saw, sah, sub, kind):
    src, refs, org = me_frames(w, h, kind)
    sad, mv = oracle.me_search(src, refs, org, saw, sah, sub)
    _freeze(sad, mv)
    return src, refs, org, sad, mv


_ZOFF = (0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15)


def me_numpy(src, refs, org, saw, sah, sub):
    """(best_sad, best_mv, ties): a scan of every position that keeps the first minimum in (y, x) order, for the 85
    blocks of every (64x64 block, reference); ties = the number of minimal positions of the 64x64 block."""
    h, w = src.shape
    nsbx = (w + 63) // 64
    nsb = nsbx * ((h + 63) // 64)
    sad = np.zeros((nsb, len(refs), 85), np.uint32)
    mv = np.zeros((nsb, len(refs), 85), np.uint32)
    ties = np.zeros((nsb, len(refs)), np.int64)
    S = src.astype(np.int64)
    for sb in range(nsb):
        sy, sx = 64 * (sb // nsbx), 64 * (sb % nsbx)
        s = S[np.ix_(np.minimum(sy + np.arange(64), h - 1), np.minimum(sx + np.arange(64), w - 1))]
        for r, ref in enumerate(refs):
            ox, oy = int(org[sb, r, 0]), int(org[sb, r, 1])
            win = ref.astype(np.int64)[np.ix_(np.clip(sy + oy + np.arange(64 + sah), 0, h - 1),
                                              np.clip(sx + ox + np.arange(64 + saw), 0, w - 1))]
            v = np.lib.stride_tricks.sliding_window_view(win, (64, 64))[:sah, :saw]  # [y][x][64][64]
            d = np.abs(v - s).reshape(sah, saw, 8, 8, 8, 8)  # [y][x][8x8 row][line][8x8 col][sample]
            s8 = 2 * d[:, :, :, 0::2].sum(axis=(3, 5)) if sub else d.sum(axis=(3, 5))  # [y][x][8][8]
            s16 = s8.reshape(sah, saw, 4, 2, 4, 2).sum(axis=(3, 5))
            s32 = s16.reshape(sah, saw, 2, 2, 2, 2).sum(axis=(3, 5))
            cols = np.zeros((sah * saw, 85), np.int64)
            for by in range(4):
                for bx in range(4):
                    q = _ZOFF[4 * by + bx]
                    cols[:, 64 + q] = s16[:, :, by, bx].ravel()
                    for k in range(4):
                        cols[:, 4 * q + k] = s8[:, :, 2 * by + (k >> 1), 2 * bx + (k & 1)].ravel()
            for k in range(4):
                cols[:, 80 + k] = s32[:, :, k >> 1, k & 1].ravel()
            cols[:, 84] = s32.sum(axis=(2, 3)).ravel()
            first = cols.argmin(axis=0)  # argmin returns the first minimum: the raveled order is (y, x)
            sad[sb, r] = cols[first, np.arange(85)]
            py, px = first // saw, first % saw
            mv[sb, r] = (((oy + py) & 0xFFFF) << 16) | ((ox + px) & 0xFFFF)
            ties[sb, r] = (cols[:, 84] == cols[:, 84].min()).sum()
    return sad, mv, ties


# --------------------------------------------------------------------------------------------- 6. CCSO search
CCSO_KINDS = ("flat_luma", "max_zero", "zero_max", "checker")
CCSO_CASES = [(w, h, bd, k) for (w, h) in ((64, 64), (136, 72)) for bd in (8, 10) for k in CCSO_KINDS]


def ccso_rd():
    """(rdmult, base_q_idx) of the first golden search case of ccso_cases.py."""
    import ccso_cases as xc
    m = xc.golden()["srch_meta"][0]
    return int(m[4]), int(m[3])


@functools.lru_cache(maxsize=None)
def ccso_case(w, h, bd, kind):
    """(pre, org[3], rec[3], (rc, params, flags, frame flag), [filtered plane] * 3) in the ccso_stride layout: uint16
    (h, w) arrays, the chroma planes in the top-left quarter."""
    import ccso_cases as xc
    o, r = {"flat_luma": ("noise", "flat"), "max_zero": ("max", "zero"), "zero_max": ("zero", "max"),
            "checker": ("anti", "checker")}[kind]
    org = [xc.full(a.astype(np.uint16), w, h) for a in planes(o, w, h, bd)]
    rec = [xc.full(a.astype(np.uint16), w, h) for a in planes(r, w, h, bd)]
    pre = rec[0].copy()  # the luma the classifier reads: flat, all zero, all max or the checkerboard
    rdmult, q = ccso_rd()
    ext = oracle.ccso_extend(pre)
    res = oracle.ccso_search_frame(ext, org, rec, bd, rdmult, q)
    outs = []
    for p in range(3):
        ph, pw = (h >> 1, w >> 1) if p else (h, w)
        pl = np.ascontiguousarray(rec[p][:ph, :pw] if bd > 8 else rec[p][:ph, :pw].astype(np.uint8))
        outs.append((pl, oracle.ccso_apply_plane(ext, bd, p, pl, res[1][p], res[2][p])))
    _freeze(pre, ext, *org, *rec, *res[2], *[a for t in outs for a in t])
    return pre, org, rec, res, outs, ext


# --------------------------------------------------------------------------------------------- 7. DLF level search
DLF_PAIRS = (("flat", "flat"), ("checker", "noise"), ("max", "zero"), ("sparse_max", "flat"))
DLF_CASES = [(w, h, bd, r, s) for (w, h) in ((64, 64), (72, 40)) for bd in (8, 10) for r, s in DLF_PAIRS]
# the builder and parameters of test_dlf_gpu.py's second PICK_CASES entry
DLF_START, DLF_PICK_ARGS, DLF_MI_SEED = (32, 32, 16, 16), (0, 0, 0, 2, 0), 15


def dlf_params():
    return svtgpu.LfParams.make(*DLF_START, ref_deltas=(1, 0, 0, 0, -1, 0, -1, -1), mode_deltas=(0, 0))


@functools.lru_cache(maxsize=None)
def dlf_case(w, h, bd, rname, sname):
    """(rec, src, mode info, picked LfParams, frame filtered at the picked levels) from the oracle."""
    import dlf_cases as dc
    rec, src = planes(rname, w, h, bd), planes(sname, w, h, bd)
    mi = dc.random_mode_info(w, h, DLF_MI_SEED, p_skip=0.3)
    picked = oracle.dlf_pick(rec, src, bd, mi, dlf_params(), *DLF_PICK_ARGS)
    out = oracle.dlf_frame(rec, bd, mi, picked)
    _freeze(mi, *rec, *src, *out)
    return rec, src, mi, picked, out


# --------------------------------------------------------------------------------------------- 8. CDEF pick
# recon against source.  A flat, black, white or checkerboard recon is left unchanged by every strength (the
# checkerboard's full-swing steps exceed every damping limit), so every searched strength of a filter block has the
# same MSE and every call of the pick ties.
CDEF_PAIRS = (("flat", "noise"), ("zero", "noise"), ("max", "noise"), ("checker", "noise"), ("flat", "flat"))
CDEF_TIED = ("flat", "zero", "max", "checker")
CDEF_LEVELS = (1, 2, 12)  # 64 strengths; 48 with the second pass's chroma at default_mse_uv * 64; 4 with the bias 62
CDEF_CASES = [(w, h, bd, lv, r, s) for (w, h) in ((64, 64), (136, 72)) for bd in (8, 10) for lv in CDEF_LEVELS
              for r, s in CDEF_PAIRS]
CDEF_Q, CDEF_LAMBDA = 128, 60000


@functools.lru_cache(maxsize=None)
def cdef_case(w, h, bd, level, rname, sname):
    """(rec, src, (mse, skip, dir, var), (parameter tuple, per-FB strengths), filtered frame) from the oracle's
    cdef_search_frame -> cdef_pick -> cdef_apply_frame."""
    rec, src = planes(rname, w, h, bd), planes(sname, w, h, bd)
    ctrls = oracle.controls(level)
    mse, skip, d, v = oracle.cdef_search_frame(rec, src, bd, ctrls, CDEF_Q)
    prm, fbs = oracle.cdef_pick(w, h, mse, skip, ctrls, CDEF_Q, CDEF_LAMBDA)
    out = oracle.cdef_apply_frame(rec, bd, None, d, v, prm, fbs)
    _freeze(*rec, *src, mse, skip, d, v, fbs, *out)
    return rec, src, (mse, skip, d, v), (prm.as_tuple(), fbs), out
