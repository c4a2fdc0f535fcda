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


def walk(padded, pad, it, wsrc, mask, cost):
    """svt_av1_obmc_full_pixel_search (av1me.c:721-776) of one item: (col, row, best_sad, variance, sse, moves).
    it: dict of PAR fields (frame / errorperbit unused); cost: the item's tables (cost_mode 1) or None."""
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
        for j, (nr, nc) in enumerate(NEIGHBORS[:8 if it["search_diag"] else 4]):
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
        row, col, moves = row + NEIGHBORS[site][0], col + NEIGHBORS[site][1], moves + 1
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
