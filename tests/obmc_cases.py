"""The OBMC fixture (tests/golden/obmc.bin, written by tests/golden/gen_golden_obmc.c from the reference's own C) and
a numpy restatement of the three OBMC kernels and of the full-pel walk.  tests/test_obmc.py holds the restatement to
every record of the fixture; tests/test_obmc_gpu.py holds the device to the fixture and to the restatement."""
import os

import numpy as np

import golden_io

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "obmc.bin")
SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32),
         (64, 64), (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
SUBPEL = [(0, 0), (4, 4), (7, 3), (0, 5)]  # (xoffset, yoffset) of blk<k>_res columns 3..10
WSRC_MAX = 255 * 4096
NEIGHBORS = [(-1, 0), (0, -1), (0, 1), (1, 0), (-1, 1), (1, 1), (1, -1), (-1, -1)]  # (row, col), av1me.c:724
MV_LOW, MV_UPP = -(1 << 14), 1 << 14
PAR = ["frame", "x", "y", "w", "h", "mvp_col", "mvp_row", "ref_mv_col", "ref_mv_row", "col_min", "col_max", "row_min",
       "row_max", "sad_per_bit", "search_range", "search_diag", "cost_mode", "errorperbit"]

_cache = {}


def fixture():
    if "g" not in _cache:
        _cache["g"] = golden_io.load(FIXTURE)
    return _cache["g"]


# ---- the kernels -------------------------------------------------------------------------------------------------
def _diff(pre, wsrc, mask):
    return wsrc.astype(np.int64) - pre.astype(np.int64) * mask.astype(np.int64)


def obmc_sad(pre, wsrc, mask):
    """sad_av1.c:18-32: sum of ROUND_POWER_OF_TWO(|wsrc - pre * mask|, 12), unsigned int."""
    return int(((np.abs(_diff(pre, wsrc, mask)) + 2048) >> 12).sum()) & 0xFFFFFFFF


def obmc_variance(pre, wsrc, mask):
    """variance.c:347-373: (variance, sse) over ROUND_POWER_OF_TWO_SIGNED(wsrc - pre * mask, 12)."""
    v = _diff(pre, wsrc, mask)
    d = np.where(v < 0, -((-v + 2048) >> 12), (v + 2048) >> 12)
    s = int(d.sum())
    sse = int((d * d).sum()) & 0xFFFFFFFF
    q = abs(s * s) // pre.size  # C division truncates; s * s >= 0
    return (sse - (q & 0xFFFFFFFF)) & 0xFFFFFFFF, sse


def bilinear(window, w, h, xoff, yoff):
    """variance.c:375-388: 2-tap bilinear of the (h + 1) x (w + 1) window, first pass to 16 bits, second to 8."""
    a = window.astype(np.int64)
    f1 = (a[:h + 1, :w] * (128 - 16 * xoff) + a[:h + 1, 1:w + 1] * (16 * xoff) + 64) >> 7
    f2 = (f1[:h] * (128 - 16 * yoff) + f1[1:h + 1] * (16 * yoff) + 64) >> 7
    return (f2 & 0xFF).astype(np.uint8)


def obmc_sub_pixel_variance(window, w, h, xoff, yoff, wsrc, mask):
    return obmc_variance(bilinear(window, w, h, xoff, yoff), wsrc, mask)


def block_case(k, case):
    """(window (h + 1, w + 1) u8, wsrc (h, w) i32, mask (h, w) i32, expected u32[11]) of size k's case 0..3."""
    g = fixture()
    w, h = (int(v) for v in g["sizes"][k])
    res = g["blk%d_res" % k][case]
    if case < 2:
        win = g["blk%d_pre" % k][case].reshape(h + 1, w + 1)
        wsrc = g["blk%d_wsrc" % k][case].reshape(h, w).astype(np.int32)
        mask = g["blk%d_mask" % k][case].reshape(h, w).astype(np.int32)
    elif case == 2:  # every diff +255
        win = g["blk%d_pre" % k][0].reshape(h + 1, w + 1)
        wsrc, mask = np.full((h, w), WSRC_MAX, np.int32), np.zeros((h, w), np.int32)
    else:  # every diff -255
        win = np.full((h + 1, w + 1), 255, np.uint8)
        wsrc, mask = np.zeros((h, w), np.int32), np.full((h, w), 4096, np.int32)
    return np.ascontiguousarray(win), wsrc, mask, res


def block_expected(win, wsrc, mask):
    """The 11 values of a blk<k>_res row from the restatement."""
    h, w = wsrc.shape
    var, sse = obmc_variance(win[:h, :w], wsrc, mask)
    out = [obmc_sad(win[:h, :w], wsrc, mask), var, sse]
    for xo, yo in SUBPEL:
        out += list(obmc_sub_pixel_variance(win, w, h, xo, yo, wsrc, mask))
    return np.array(out, np.uint32)


# ---- the walk ----------------------------------------------------------------------------------------------------
def pad_frame(frame, pad=192):
    """Edge replication: a sample outside the frame reads the nearest edge sample."""
    return np.pad(frame, pad, mode="edge"), pad


def cost_tables(it, joint, comp_row, comp_col):
    """The batch's cost tables of an item (include/svtgpu.h) from centred full tables comp_*[v + MV_UPP]."""
    R = it["search_range"]
    sr = min(max(it["mvp_row"], it["row_min"]), it["row_max"])
    sc = min(max(it["mvp_col"], it["col_min"]), it["col_max"])
    clip = lambda v: min(max(v, MV_LOW), MV_UPP)
    rows = [comp_row[clip((sr - R + k - (it["ref_mv_row"] >> 3)) * 8) + MV_UPP] for k in range(2 * R + 1)]
    cols = [comp_col[clip((sc - R + k - (it["ref_mv_col"] >> 3)) * 8) + MV_UPP] for k in range(2 * R + 1)]
    return np.array(list(joint) + rows + cols, np.int32)


def walk(padded, pad, it, wsrc, mask, cost, neighbors=None):
    """svt_av1_obmc_full_pixel_search (av1me.c:721-776) of one item: (col, row, best_sad, variance, sse, moves).
    it: dict of PAR fields (frame / errorperbit unused); cost: the item's tables (cost_mode 1) or None.  neighbors (tests
    only): another order of the eight sites than the reference's."""
    neighbors = NEIGHBORS if neighbors is None else neighbors
    w, h, R = it["w"], it["h"], it["search_range"]
    fr, fc = it["ref_mv_row"] >> 3, it["ref_mv_col"] >> 3
    sr = min(max(it["mvp_row"], it["row_min"]), it["row_max"])
    sc = min(max(it["mvp_col"], it["col_min"]), it["col_max"])
    T = 2 * R + 1

    def pre(row, col):
        y, x = it["y"] + row + pad, it["x"] + col + pad
        return padded[y:y + h, x:x + w]

    def mv_cost(row, col):
        dr, dc = row - fr, col - fc
        if it["cost_mode"] == 0:  # mvsad_err_cost_light
            return (1296 + 50 * (abs(dc) * 8 + abs(dr) * 8)) & 0xFFFFFFFF
        j = (0 if dc == 0 else 1) if dr == 0 else (2 if dc == 0 else 3)
        bits = (int(cost[j]) + int(cost[4 + row - (sr - R)]) + int(cost[4 + T + col - (sc - R)])) & 0xFFFFFFFF
        return (((bits * it["sad_per_bit"]) & 0xFFFFFFFF) + 256 & 0xFFFFFFFF) >> 9

    row, col, moves = sr, sc, 0
    best = (obmc_sad(pre(row, col), wsrc, mask) + mv_cost(row, col)) & 0xFFFFFFFF
    for _ in range(R):
        site = -1
        for j, (nr, nc) in enumerate(neighbors[:8 if it["search_diag"] else 4]):
            r, c = row + nr, col + nc
            if not (it["col_min"] <= c <= it["col_max"] and it["row_min"] <= r <= it["row_max"]):
                continue
            sad = obmc_sad(pre(r, c), wsrc, mask)
            if sad < best:
                sad = (sad + mv_cost(r, c)) & 0xFFFFFFFF
                if sad < best:
                    best, site = sad, j
        if site < 0:
            break
        row, col, moves = row + neighbors[site][0], col + neighbors[site][1], moves + 1
    var, sse = obmc_variance(pre(row, col), wsrc, mask)
    return col, row, best, var, sse, moves


def walk_cases():
    """[(item dict, wsrc (h, w) i32, mask (h, w) i32, cost tables or None, res i32[5])] of the fixture."""
    g = fixture()
    out = []
    for i in range(int(g["walk_count"][0])):
        it = {k: int(v) for k, v in zip(PAR, g["walk%d_par" % i])}
        shape = (it["h"], it["w"])
        wsrc = g["walk%d_wsrc" % i].reshape(shape).astype(np.int32)
        mask = g["walk%d_mask" % i].reshape(shape).astype(np.int32)
        out.append((it, wsrc, mask, g.get("walk%d_cost" % i), g["walk%d_res" % i]))
    return out


# ---- a mixed batch for the device test: 192 x 136, 2 references -------------------------------------------------------
def mixed_batch(seed=0x0B3C):
    """(frames [2] u8 (136, 192), items [dict], wsrc list, mask list, cost list) -- about 40 items: the listed sizes,
    blocks on all four frame edges, both cost modes, both range / diag settings, limits that clip."""
    rng = np.random.default_rng(seed)
    W, H = 192, 136
    frames = []
    for r in range(2):  # smooth content, so walks run for several steps
        yy, xx = np.mgrid[0:H, 0:W]
        f = 128 + 70 * np.sin(xx / (9.0 + 3 * r)) * np.cos(yy / (7.0 + 2 * r)) + rng.integers(-6, 7, (H, W))
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
    joint = [310, 1187, 1243, 1920]
    v = np.arange(MV_LOW, MV_UPP + 1)
    comp = [(400 + 37 * np.floor(np.log2(np.abs(v) + 1)) * 8 + (np.abs(v) * (13 + 4 * c)) % 29).astype(np.int64)
            for c in range(2)]
    sizes = [(4, 4), (4, 16), (16, 4), (8, 8), (16, 16), (32, 8), (64, 64), (64, 128), (128, 64), (128, 128)]
    items, wsrcs, masks, costs = [], [], [], []
    for n in range(40):
        w, h = sizes[n % len(sizes)]
        corner = (n // len(sizes)) % 4  # walk the four frame edges
        x = [0, W - w, int(rng.integers(0, (W - w) // 4 + 1)) * 4, W - 4][corner]
        y = [int(rng.integers(0, (H - h) // 4 + 1)) * 4, 0, H - h, H - 4][corner]
        x, y = min(x, W - 1), min(y, H - 1)
        ref = n % 2
        mode, (R, diag) = (n // 2) % 2, [(16, 1), (8, 0)][(n // 4) % 2]
        lim = 6 if n % 5 == 0 else 48  # every fifth item: limits that clip the walk
        tx, ty = (int(t) for t in rng.integers(-9, 10, 2))
        padded, pad = pad_frame(frames[ref])
        mask = rng.integers(1024, 4097, (h, w)).astype(np.int32)
        tgt = padded[y + ty + pad:y + ty + pad + h, x + tx + pad:x + tx + pad + w].astype(np.int64)
        wsrc = np.clip(tgt * mask + rng.integers(-800, 801, (h, w)), 0, WSRC_MAX).astype(np.int32)
        it = dict(frame=ref, x=x, y=y, w=w, h=h, mvp_col=int(rng.integers(-12, 13)), mvp_row=int(rng.integers(-12, 13)),
                  ref_mv_col=int(rng.integers(-90, 91)), ref_mv_row=int(rng.integers(-90, 91)), col_min=-lim,
                  col_max=lim - 1, row_min=-lim + 2, row_max=lim, sad_per_bit=int(rng.integers(20, 120)),
                  search_range=R, search_diag=diag, cost_mode=mode, errorperbit=0)
        items.append(it)
        wsrcs.append(wsrc)
        masks.append(mask)
        costs.append(cost_tables(it, joint, comp[0], comp[1]) if mode else None)
    return frames, items, wsrcs, masks, costs


# ---- tie and full-magnitude content for the device test: 192 x 136 ------------------------------------------------------
EXTREME_SIZES = [(4, 4), (16, 16), (64, 64), (128, 128)]
CORNER_X, CORNER_Y = 150, 130  # full magnitude: the frame is 255 from here to its far corner, 0 elsewhere
SWAPPED = {"v_stripes": [NEIGHBORS[k] for k in (0, 2, 1, 3, 4, 5, 6, 7)],  # the tied pair (0, -1) / (0, 1) swapped
           "h_stripes": [NEIGHBORS[k] for k in (3, 1, 2, 0, 4, 5, 6, 7)]}  # the tied pair (-1, 0) / (1, 0) swapped


def extreme_batch():
    """(frames [4] u8 (136, 192), items, wsrc list, mask list, cost list, kinds): 24 items of the sizes 4x4, 16x16, 64x64 and
    128x128, both cost modes, search_diag 0 (range 8) and 1 (range 16).  One frame per content (the batch takes up to 8):
      flat (frame 0, all 128): every neighbour's SAD equals the start's; the start is the centre of the MV cost
        (ref_mv = 8 * the clamped start), so no neighbour is cheaper either: 0 steps, the result is the clamped start.
        Every second item's mvp lies outside its limits.
      v_stripes / h_stripes (frames 1, 2: period 4, two samples of 255 and two of 0), wsrc = 4096 * the frame displaced by
        2 samples (half a period) across the stripes, mask 4096, start = ref_mv = 0: the start sees the inverse, the two
        neighbours across the stripes see half of it and tie, in SAD and in cost; the first in NEIGHBORS order takes over
        and the next step ends on SAD 0, two samples to that side.  (The neighbours along the stripes tie too, with each
        other and with the position itself, but cost more than it: they never take over.)
      full (frame 3: 0, but 255 at x >= CORNER_X, y >= CORNER_Y), wsrc = WSRC_MAX, mask 4096: SAD = sum of 255 - pre.  The
        block starts with its last row just above the corner, 255 * w * h exactly (128x128: 4 177 920), its columns
        overlapping the corner's, so every step down takes 255 * overlap off.  With cost mode 1 the tables are times 1024
        and sad_per_bit is 6000: bits * sad_per_bit passes 2^32 and wraps as the reference's unsigned product does."""
    W, H = 192, 136
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [np.full((H, W), 128, np.uint8), (((xx >> 1) & 1) * 255).astype(np.uint8), (((yy >> 1) & 1) * 255).astype(np.uint8),
              np.where((xx >= CORNER_X) & (yy >= CORNER_Y), 255, 0).astype(np.uint8)]
    rng = np.random.default_rng(0x0B3D)
    joint = [310, 1187, 1243, 1920]
    v = np.arange(MV_LOW, MV_UPP + 1)
    comp = [(400 + 37 * np.floor(np.log2(np.abs(v) + 1)) * 8 + (np.abs(v) * (13 + 4 * c)) % 29).astype(np.int64) for c in range(2)]
    items, wsrcs, masks, costs, kinds = [], [], [], [], []

    def add(kind, frame, x, y, w, h, mvp, ref_mv, lim, mode, diag, wsrc, mask, spb=60, scale=1):
        it = dict(frame=frame, x=x, y=y, w=w, h=h, mvp_col=mvp[0], mvp_row=mvp[1], ref_mv_col=ref_mv[0], ref_mv_row=ref_mv[1],
                  col_min=lim[0], col_max=lim[1], row_min=lim[2], row_max=lim[3], sad_per_bit=spb, search_range=16 if diag else 8,
                  search_diag=diag, cost_mode=mode, errorperbit=0)
        items.append(it), wsrcs.append(wsrc.astype(np.int32)), masks.append(mask.astype(np.int32)), kinds.append(kind)
        costs.append(cost_tables(it, [j * scale for j in joint], comp[0] * scale, comp[1] * scale) if mode else None)

    for k, (w, h) in enumerate(EXTREME_SIZES):
        for mode in (0, 1):
            diag, n = (k + mode) & 1, len(items)
            mvp, lim = ((5 - k, k - 3), (-20, 19, -18, 20)) if n & 1 == 0 else ((60 + k, -70), (-20, 19, -18, 20))
            start = (min(max(mvp[0], lim[0]), lim[1]), min(max(mvp[1], lim[2]), lim[3]))
            mask = rng.integers(1024, 4097, (h, w))
            add("flat", 0, 32, 4, w, h, mvp, (8 * start[0], 8 * start[1]), lim, mode, diag,
                np.clip(128 * mask + rng.integers(-90000, 90001, (h, w)), 0, WSRC_MAX), mask)
    for kind, frame in (("v_stripes", 1), ("h_stripes", 2)):
        for k, (w, h) in enumerate(EXTREME_SIZES):
            x, y = 32, 4
            dx, dy = (2, 0) if frame == 1 else (0, 2)
            add(kind, frame, x, y, w, h, (0, 0), (0, 0), (-20, 19, -18, 20), k & 1, k >> 1 & 1,
                4096 * frames[frame][y + dy:y + dy + h, x + dx:x + dx + w].astype(np.int64), np.full((h, w), 4096))
    for k, (w, h) in enumerate(EXTREME_SIZES):
        for mode in (0, 1):
            x, y = min(152, W - w), CORNER_Y - h - 2
            add("full", 3, x, y, w, h, (0, 2), (0, 16), (-48, 47, -46, 48), mode, (k + mode) & 1, np.full((h, w), WSRC_MAX),
                np.full((h, w), 4096), spb=6000 if mode else 60, scale=1024 if mode else 1)
    return frames, items, wsrcs, masks, costs, kinds


def pack(items, wsrcs, masks, costs):
    """(item rows for svtgpu.ObmcBatch.set_items, wm pool, cost pool): offsets assigned in list order."""
    wm, cp, rows = [], [], []
    woff = coff = 0
    for it, ws, mk, ct in zip(items, wsrcs, masks, costs):
        rows.append(dict(it, ref=it["frame"], wm_offset=woff, cost_offset=coff if ct is not None else 0))
        wm += [ws.reshape(-1), mk.reshape(-1)]
        woff += 2 * ws.size
        if ct is not None:
            cp.append(np.asarray(ct, np.int32))
            coff += len(ct)
    return (rows, np.concatenate(wm).astype(np.int32),
            np.concatenate(cp).astype(np.int32) if cp else np.zeros(0, np.int32))
