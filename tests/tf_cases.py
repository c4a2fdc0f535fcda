"""The temporal filter's filter half: reader of tests/golden/tf.bin (written by tests/golden/gen_golden_tf.c from the
reference's own C) and a numpy restatement of EbTemporalFiltering.c's noise estimate (:3672-3740), centre seeding
(:353-425), planewise weighting and accumulation (:793-1365), normalisation (:2582-2646) and the block walk of
produce_temporally_filtered_pic (:2939-3301).  Shared by tests/test_tf.py (CPU) and tests/test_tf_gpu.py."""
import functools
import os

import numpy as np

import golden_io

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tf.bin")
M32 = 0xFFFFFFFF
_C = 0x9E3779B97F4A7C15


@functools.lru_cache(maxsize=1)
def fixture():
    return golden_io.load(GOLDEN)


def draw(seed, n, mod):
    """Samples 0..n-1 of the generator's stream `seed`: SplitMix64(seed + (i + 1) * C) % mod."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(_C)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(mod)).astype(np.int64)


# ---------------------------------------------------------------------------------------------
# scalar arithmetic
# ---------------------------------------------------------------------------------------------
def tables():
    g = fixture()
    return g["tab_log1p"], g["tab_sqrt"], g["tab_expf"]


def noise_log1p_fp16(noise_level_fp16):
    log1p, _, _ = tables()
    base = 65536 + int(noise_level_fp16)
    if base <= 0:
        return -2147483648
    if base < 458752:
        i, rest = base >> 11, base & 0x7FF
        return int(log1p[i]) + ((rest * (int(log1p[i + 1]) - int(log1p[i]))) >> 11)
    return ((1860 * (int(noise_level_fp16) >> 8)) >> 8) + 116456


def _cdiv(a, b):  # C's division: towards zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def decay_factor_fp16(decay_control, noise_log1p, q):
    q_decay = (q * q) >> 5 if q >= 128 else max(q << 2, 1)
    n_decay = _cdiv(decay_control * (45875 + noise_log1p), 64)
    return ((n_decay * n_decay * q_decay) >> 11) & M32


def sqrt_fast(x):
    _, sq, _ = tables()
    if x > 15:
        half = (x.bit_length() - 1) >> 1
        return int(sq[x >> (2 * half - 2)]) >> (17 - half)
    return int(sq[x]) >> 16


def d_factor_fp8(col, row, mv_dist_th):
    thr = max((mv_dist_th << 16) // 10, 1 << 16)
    dist = sqrt_fast(((col * col + row * row) << 8) & M32)
    return max(((dist << 12) & M32) // (thr >> 8), 256)


def window_error(sse, half, bd):
    s = (int(sse) & M32) >> (2 * (bd - 8))
    return (((((s << 4) & M32) // half) << 4) & M32) // half


def quadrant_weights(meta, idx, q, decay, mv_dist_th, bd, zz, win, luma_win):
    """The weight of quadrant q of 32x32 block idx for one plane.  win: the plane's own window error (None for zz);
    luma_win: the luma window error when the plane is chroma, else None.  Returns (weight, scaled_diff16, wide)."""
    _, _, expf = tables()
    split = int(meta["split"][idx])
    if split:
        be = int(meta["err16"][idx * 4 + q]) >> (4 if bd > 8 else 0)
        col, row = (int(v) for v in meta["mv16"][idx * 4 + q])
    else:
        be = int(meta["err32"][idx]) >> (6 if bd > 8 else 2)
        col, row = (int(v) for v in meta["mv32"][idx])
    be &= M32
    if zz:
        sd = min(((be << 2) & M32) // max(decay >> 10, 1), 112)
        return (int(expf[sd]) * 1000) >> 17, sd, False
    if not split:
        decay = (decay << 1) & M32
    if luma_win is not None:
        win = ((win * 5 + luma_win) & M32) // 6
    comb = ((win * 5 + be) & M32) // 6
    d = d_factor_fp8(col, row, mv_dist_th)
    prod = (comb >> 3) * (d >> 3)
    sd = min((prod & M32) // max(decay >> 10, 1), 112)
    return (int(expf[sd]) * 1000) >> 16, sd, prod > M32


def apply_block(meta, idx, src, pre, accum, count, decay, mv_dist_th, tf_chroma, bd, zz, stats=None):
    """One svt_av1_apply_(zz_based_)temporal_filter_planewise_medium(_hbd) call: src / pre are three [bh][bw] planes
    (chroma halved), accum / count are updated in place (uint32 / uint16 arithmetic)."""
    luma = [0] * 4
    for p in range(3 if tf_chroma else 1):
        hh, hw = src[p].shape[0] // 2, src[p].shape[1] // 2
        for q in range(4):
            ys, xs = slice((q >> 1) * hh, (q >> 1) * hh + hh), slice((q & 1) * hw, (q & 1) * hw + hw)
            win = None
            if not zz:
                d = src[p][ys, xs].astype(np.int64) - pre[p][ys, xs].astype(np.int64)
                win = window_error((d * d).sum(), hw, bd)
                if p == 0:
                    luma[q] = win
            w, sd, wide = quadrant_weights(meta, idx, q, int(decay[p]), mv_dist_th, bd, zz, win, luma[q] if p else None)
            if stats is not None:
                stats.append((sd, w, wide))
            count[p][ys, xs] = (count[p][ys, xs].astype(np.int64) + w).astype(np.uint16)
            accum[p][ys, xs] = (accum[p][ys, xs].astype(np.int64) + w * pre[p][ys, xs].astype(np.int64)).astype(np.uint32)


def central(src, tf_chroma):
    accum = [np.zeros(s.shape, np.uint32) for s in src]
    count = [np.zeros(s.shape, np.uint16) for s in src]
    for p in range(3 if tf_chroma else 1):
        accum[p][:] = 1000 * src[p].astype(np.uint32)
        count[p][:] = 1000
    return accum, count


def final(accum, count):
    a, c = accum.astype(np.int64), count.astype(np.int64)
    return (a + (c >> 1)) // c


def estimate_noise(plane, bd):
    """(result, num) of svt_estimate_noise_fp16_c / svt_estimate_noise_highbd_fp16_c."""
    s = plane.astype(np.int64)
    h, w = s.shape
    if h < 3 or w < 3:
        return -65536, 0
    a, b, c = s[:-2, :-2], s[:-2, 1:-1], s[:-2, 2:]
    d, e, f = s[1:-1, :-2], s[1:-1, 1:-1], s[1:-1, 2:]
    g, hh, i = s[2:, :-2], s[2:, 1:-1], s[2:, 2:]
    gx = (a - c) + (g - i) + 2 * (d - f)
    gy = (a - g) + (c - i) + 2 * (b - hh)
    sh = bd - 8
    rnd = (1 << sh) >> 1
    ga = (np.abs(gx) + np.abs(gy) + rnd) >> sh
    v = (np.abs(4 * e - 2 * (d + f + b + hh) + (a + c + g + i)) + rnd) >> sh
    m = ga < 50
    num, tot = int(m.sum()), int(v[m].sum())
    return (-65536 if num < 16 else (tot * 82137) // (6 * num)), num


def block_index(bx, by, blk_cols):
    return by * blk_cols + bx


def filter_frame(centre, refs, metas, decay, mv_dist_th, tf_chroma, bd, zz, w, h, stats=None):
    """produce_temporally_filtered_pic's block loop over planes given on the 64-aligned area; metas[r][blk] is the
    metadata of reference r, block blk.  Returns the three filtered planes (aligned area)."""
    out = [c.copy() for c in centre]
    bc, br = (w + 63) // 64, (h + 63) // 64
    for by in range(br):
        for bx in range(bc):
            def blk(pl, p):
                s = 64 >> (p > 0)
                return pl[by * s:by * s + s, bx * s:bx * s + s]
            src = [blk(centre[p], p) for p in range(3)]
            accum, count = central(src, tf_chroma)
            for r, ref in enumerate(refs):
                pre = [blk(ref[p], p) for p in range(3)]
                meta = metas[r][block_index(bx, by, bc)]
                for idx in range(4):
                    def sub(a, p):
                        s = 32 >> (p > 0)
                        return a[(idx >> 1) * s:(idx >> 1) * s + s, (idx & 1) * s:(idx & 1) * s + s]
                    apply_block(meta, idx, [sub(src[p], p) for p in range(3)], [sub(pre[p], p) for p in range(3)],
                                [sub(accum[p], p) for p in range(3)], [sub(count[p], p) for p in range(3)], decay,
                                mv_dist_th, tf_chroma, bd, zz, stats)
            for p in range(3 if tf_chroma else 1):
                blk(out[p], p)[:] = final(accum[p], count[p]).astype(out[p].dtype)
    return out


# ---------------------------------------------------------------------------------------------
# the fixture's records
# ---------------------------------------------------------------------------------------------
def dtype_of(bd):
    return np.uint16 if bd > 8 else np.uint8


def noise_plane(bd, w, h, seed):
    """content 0 of the generator (the only drawn noise content)."""
    sc = 1 << (bd - 8)
    y, x = np.mgrid[0:h, 0:w]
    v = (x + 2 * y) * sc // 8 + draw(0x5446000000000100 + seed, w * h, 10 * sc).reshape(h, w)
    return np.clip(v, 0, (1 << bd) - 1).astype(dtype_of(bd))


def noise_cases():
    g = fixture()
    for i in range(int(g["nnoise"][0])):
        bd, w, h, content, seed = (int(v) for v in g["n%d_par" % i])
        src = g["n%d_src" % i] if "n%d_src" % i in g else noise_plane(bd, w, h, seed)
        yield dict(name="noise%d %d-bit %dx%d content %d" % (i, bd, w, h, content), bd=bd, w=w, h=h, content=content,
                   src=src, out=int(g["n%d_out" % i][0]))


def _meta(g, pre):
    return dict(split=g[pre + "_split"], mv32=g[pre + "_mv32"], mv16=g[pre + "_mv16"], err32=g[pre + "_err32"],
                err16=g[pre + "_err16"])


def block_cases():
    g = fixture()
    for i in range(int(g["nblock"][0])):
        bd, bw, zz, chroma, idx, th, content, prefill, n, meta, decayset = (int(v) for v in g["b%d_par" % i])
        maxv, sc, seed = (1 << bd) - 1, 1 << (bd - 8), 0x5446000000001000 + 16 * n
        src, pre = [], []
        for p in range(3):
            w = bw >> (p > 0)
            s = draw(seed + p, w * w, maxv + 1)
            if content == 0:
                q = np.clip(s - 16 * sc + draw(seed + 4 + p, w * w, 32 * sc), 0, maxv)
            elif content == 1:
                q = draw(seed + 4 + p, w * w, maxv + 1)
            elif content == 2:
                s, q = np.zeros_like(s), np.full_like(s, maxv)
            else:
                s, q = np.full_like(s, maxv), np.zeros_like(s)
            src.append(s.reshape(w, w).astype(dtype_of(bd)))
            pre.append(q.reshape(w, w).astype(dtype_of(bd)))
        accum = [np.zeros(s.shape, np.uint32) for s in src]
        count = [np.zeros(s.shape, np.uint16) for s in src]
        if prefill:
            accum, count = central(src, chroma)
        yield dict(name="block%d %d-bit bw %d zz %d chroma %d idx %d th %d content %d prefill %d meta %d decay %d" %
                   (i, bd, bw, zz, chroma, idx, th, content, prefill, meta, decayset), bd=bd, bw=bw, zz=zz,
                   tf_chroma=chroma, idx=idx, mv_dist_th=th, content=content, prefill=prefill, metaset=meta,
                   decay=g["b%d_decay" % i], meta=_meta(g, "b%d" % i), src=src, pre=pre, accum_in=accum, count_in=count,
                   wide=int(g["b%d_wide" % i][0]), accum=[g["b%d_accum%d" % (i, p)] for p in range(3)],
                   count=[g["b%d_count%d" % (i, p)] for p in range(3)])


CS = 80  # the luma stride of the central / final records


def central_cases():
    g = fixture()
    for i in range(int(g["ncentral"][0])):
        bd, chroma, n = (int(v) for v in g["c%d_par" % i])
        seed = 0x5446000000002000 + 16 * n
        src = [draw(seed + p, (64 >> (p > 0)) ** 2, 1 << bd).reshape(64 >> (p > 0), -1).astype(dtype_of(bd)) for p in range(3)]
        yield dict(name="central%d %d-bit chroma %d" % (i, bd, chroma), bd=bd, tf_chroma=chroma, src=src,
                   accum=[g["c%d_accum%d" % (i, p)] for p in range(3)], count=[g["c%d_count%d" % (i, p)] for p in range(3)])


def final_cases():
    g = fixture()
    for i in range(int(g["nfinal"][0])):
        bd, mode, n = (int(v) for v in g["e%d_par" % i])
        seed, maxv = 0x5446000000003000 + 16 * n, (1 << bd) - 1
        accum, count = [], []
        for p in range(3):
            k = (64 >> (p > 0)) ** 2
            v = draw(seed + p, k, maxv)
            c = 1000 + draw(seed + 4 + p, k, 26001) if mode else np.full(k, 1000, np.int64)
            a = v * c + (draw_each(seed + 8 + p, c) if mode else 0)
            accum.append(a.astype(np.uint32).reshape(64 >> (p > 0), -1))
            count.append(c.astype(np.uint16).reshape(64 >> (p > 0), -1))
        yield dict(name="final%d %d-bit mode %d" % (i, bd, mode), bd=bd, mode=mode, accum=accum, count=count,
                   out=[g["e%d_out%d" % (i, p)] for p in range(3)])


def draw_each(seed, mods):
    """draw with a modulus per sample."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, len(mods) + 1, dtype=np.uint64) * np.uint64(_C)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % mods.astype(np.uint64)).astype(np.int64)


def frame_pictures(bd, seed, n_refs, aw=192, ah=128):
    """The generator's drawn centre and predictor pictures over the aligned area."""
    maxv, sc = (1 << bd) - 1, 1 << (bd - 8)
    centre, refs = [], [[] for _ in range(n_refs)]
    for p in range(3):
        w, h = aw >> (p > 0), ah >> (p > 0)
        y, x = np.mgrid[0:h, 0:w]
        v = np.clip((2 * x + y) * sc // 4 + draw(seed + p, w * h, 64 * sc).reshape(h, w), 0, maxv)
        centre.append(v.astype(dtype_of(bd)))
        for r in range(n_refs):
            amp = (2 + 3 * r) * sc
            refs[r].append(np.clip(v - amp + draw(seed + 4 + 4 * r + p, w * h, 2 * amp + 1).reshape(h, w), 0,
                                   maxv).astype(dtype_of(bd)))
    return centre, refs


def frame_cases():
    g = fixture()
    for i in range(int(g["nframe"][0])):
        bd, w, h, nr, zz, chroma, th, n = (int(v) for v in g["f%d_par" % i])
        centre, refs = frame_pictures(bd, 0x5446000000005000 + 256 * n, nr)
        m = _meta(g, "f%d" % i)
        nblk = ((w + 63) // 64) * ((h + 63) // 64)
        metas = [[{k: v[r][b] for k, v in m.items()} for b in range(nblk)] for r in range(nr)]
        yield dict(name="frame%d %d-bit %dx%d refs %d zz %d chroma %d th %d" % (i, bd, w, h, nr, zz, chroma, th), bd=bd,
                   w=w, h=h, n_refs=nr, zz=zz, tf_chroma=chroma, mv_dist_th=th, decay=g["f%d_decay" % i], centre=centre,
                   refs=refs, metas=metas, out=[g["f%d_out%d" % (i, p)] for p in range(3)])


def random_metas(rng, n_refs, nblk, bd):
    sh = 4 if bd > 8 else 0
    out = []
    for _ in range(n_refs):
        row = []
        for _ in range(nblk):
            row.append(dict(split=rng.integers(0, 2, 4).astype(np.int32),
                            mv32=rng.integers(-40, 41, (4, 2)).astype(np.int16),
                            mv16=rng.integers(-40, 41, (16, 2)).astype(np.int16),
                            err32=(rng.integers(0, 200000, 4).astype(np.uint64) << np.uint64(sh)),
                            err16=(rng.integers(0, 60000, 16).astype(np.uint64) << np.uint64(sh))))
        out.append(row)
    return out
