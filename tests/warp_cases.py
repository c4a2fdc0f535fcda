"""Warped-motion prediction restated in numpy (test infrastructure): svt_get_shear_params, svt_av1_warp_affine_c /
svt_av1_highbd_warp_affine_c and svt_aom_warped_motion_prediction (no masked compound) as tests/golden/warp.bin records
them, and the inputs the fixture does not store, rebuilt from its seeds.  tests/test_warp.py holds this file to every record;
tests/test_warp_gpu.py uses it beyond the records."""
import functools
import os

import numpy as np

import golden_io
from tf_cases import draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp.bin")
NO_REF = 0xFF


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN)


def table():
    return fixture()["filter"].astype(np.int64)


# ---------------------------------------------------------------------------------------------
# svt_get_shear_params
# ---------------------------------------------------------------------------------------------
def _round_signed(v, n):
    half = (1 << n) >> 1
    return -((-v + half) >> n) if v < 0 else (v + half) >> n


def _clamp16(v):
    return max(-32768, min(32767, v))


def _i16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _i32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def shear_params(mat, div_lut=None):
    """(return value, [alpha, beta, gamma, delta]) of svt_get_shear_params; the four are zero for mat[2] <= 0, as a zeroed
    model leaves them."""
    lut = fixture()["div_lut"] if div_lut is None else div_lut
    m = [int(v) for v in mat]
    if m[2] <= 0:
        return 0, [0, 0, 0, 0]
    msb = m[2].bit_length() - 1
    e = m[2] - (1 << msb)
    f = (e + ((1 << (msb - 8)) >> 1)) >> (msb - 8) if msb > 8 else e << (8 - msb)
    y, shift = int(lut[f]), msb + 14
    alpha, beta = _clamp16(m[2] - 65536), _clamp16(m[3])
    gamma = _clamp16(_i32(_round_signed(m[4] * 65536 * y, shift)))
    delta = _clamp16(m[5] - _i32(_round_signed(m[3] * m[4] * y, shift)) - 65536)
    abgd = [_i16(_round_signed(v, 6) * 64) for v in (alpha, beta, gamma, delta)]
    ok = 4 * abs(abgd[0]) + 7 * abs(abgd[1]) < 65536 and 4 * abs(abgd[2]) + 4 * abs(abgd[3]) < 65536
    return int(ok), abgd


# ---------------------------------------------------------------------------------------------
# the two C functions
# ---------------------------------------------------------------------------------------------
def horiz_bits(bd, round_0, highbd):
    return round_0 + max(bd + 7 - round_0 - 14, 0) if highbd else round_0


def warp_sums(mat, abgd, ref, p_col, p_row, p_width, p_height, ss_x, ss_y, bd, rbh, stats=None):
    """The vertical filter's sums (offset included, unrounded) of a p_height x p_width block; `ref` is the whole plane.
    stats, if given, collects the filter rows used: stats["h"], stats["v"] sets, and the intermediate's min / max."""
    T = table()
    ref = np.asarray(ref, dtype=np.int64)
    height, width = ref.shape
    alpha, beta, gamma, delta = [int(v) for v in abgd]
    m = [int(v) for v in mat]
    out = np.zeros((p_height, p_width), np.int64)
    for i in range(p_row, p_row + p_height, 8):
        for j in range(p_col, p_col + p_width, 8):
            src_x, src_y = (j + 4) << ss_x, (i + 4) << ss_y
            dst_x, dst_y = _i32(m[2] * src_x + m[3] * src_y + m[0]), _i32(m[4] * src_x + m[5] * src_y + m[1])
            x4, y4 = dst_x >> ss_x, dst_y >> ss_y
            ix4, iy4 = x4 >> 16, y4 >> 16
            sx4 = ((x4 & 65535) - 4 * alpha - 4 * beta) & ~63
            sy4 = ((y4 & 65535) - 4 * gamma - 4 * delta) & ~63
            rows = np.clip(iy4 - 7 + np.arange(15), 0, height - 1)
            cols = np.clip(ix4 - 7 + np.arange(15), 0, width - 1)
            patch = ref[np.ix_(rows, cols)]                                     # [15][15]
            k, l = np.arange(15)[:, None], np.arange(8)[None, :]
            offs = ((sx4 + beta * (k - 3) + alpha * l + 512) >> 10) + 64        # [15][8]
            win = np.stack([patch[:, t:t + 8] for t in range(8)], axis=2)       # [15][8][8]: [k][l][tap]
            tmp = ((1 << (bd + 6)) + (win * T[offs]).sum(2) + ((1 << rbh) >> 1)) >> rbh
            k, l = np.arange(8)[:, None], np.arange(8)[None, :]
            offv = ((sy4 + delta * k + gamma * l + 512) >> 10) + 64             # [8][8]
            col = np.stack([tmp[t:t + 8, :] for t in range(8)], axis=2)         # [8][8][8]: [k][l][tap]
            out[i - p_row:i - p_row + 8, j - p_col:j - p_col + 8] = (1 << (bd + 14 - rbh)) + (col * T[offv]).sum(2)
            if stats is not None:
                stats.setdefault("h", set()).update(offs.ravel().tolist())
                stats.setdefault("v", set()).update(offv.ravel().tolist())
                stats["tmp"] = (min(stats.get("tmp", (1 << 30, 0))[0], int(tmp.min())), max(stats.get("tmp", (0, 0))[1], int(tmp.max())))
    return out


def _rnd(v, n):
    return (v + ((1 << n) >> 1)) >> n


def single(sums, bd, rbh):
    return np.clip(_rnd(sums, 14 - rbh) - (1 << (bd - 1)) - (1 << bd), 0, (1 << bd) - 1)


def average(conv, sums, bd, round_0, round_1, dist_wtd, fwd, bck):
    conv, s = np.asarray(conv, dtype=np.int64), _rnd(sums, round_1)
    t = (conv * fwd + s * bck) >> 4 if dist_wtd else (conv + s) >> 1
    ob = bd + 14 - round_0
    t = t - (1 << (ob - round_1)) - (1 << (ob - round_1 - 1))
    return np.clip(_rnd(t, 14 - round_0 - round_1), 0, (1 << bd) - 1)


def conv_rounds(bd, is_compound):
    """get_conv_params_no_round (convolve.h:40-64): (round_0, round_1)."""
    extra = max(bd + 7 - 3 + 2 - 16, 0)
    return 3 + extra, 7 if is_compound else 11 - extra


# ---------------------------------------------------------------------------------------------
# unit records
# ---------------------------------------------------------------------------------------------
def unit_plane(c, s):
    """The reference plane of pass s of unit record c (int64 [h][w])."""
    bd, w, h, content = c["bd"], c["rw"], c["rh"], c["content"]
    maxv = (1 << min(bd, 10)) - 1  # the split 8 + 2 layout holds ten bits at any bd
    if content == 0:
        return draw(0x5750000000000000 + 16 * c["index"] + 8 * s, w * h, maxv + 1).reshape(h, w).astype(np.int64)
    if content in (1, 2):
        return np.full((h, w), 0 if content == 1 else maxv, np.int64)
    pos = table()[96] > 0  # max where the half-sample row's tap is positive; pass 1 inverted; `flip` inverts both
    y, x = np.mgrid[0:h, 0:w]
    return np.where(pos[(x if content == 3 else y) & 7] ^ bool(s != c["flip"]), maxv, 0).astype(np.int64)


def unit_cases():
    g = fixture()
    out = []
    for i in range(int(g["nunit"][0])):
        p = [int(v) for v in g["u%d_par" % i]]
        c = dict(zip(("bd", "rw", "rh", "p_col", "p_row", "pw", "ph", "ss", "mode", "content", "model", "model2", "fwd", "bck", "index", "flip"), p))
        c.update(name="u%d_%dx%d_bd%d_ss%d_mode%d_c%d_m%d" % (i, c["pw"], c["ph"], c["bd"], c["ss"], c["mode"], c["content"], c["model"]),
                 mat=g["u%d_mat" % i], abgd=g["u%d_abgd" % i], out=g["u%d_out" % i], conv=g.get("u%d_conv" % i))
        out.append(c)
    return out


def unit_expected(c, stats=None):
    """(pixels, CONV_BUF_TYPE block or None) of unit record c by the restatement."""
    bd, hbd = c["bd"], c["bd"] > 8
    r0, r1 = conv_rounds(bd, c["mode"] != 0)
    rbh = horiz_bits(bd, r0, hbd)
    args = (c["p_col"], c["p_row"], c["pw"], c["ph"], c["ss"], c["ss"], bd, rbh, stats)
    s0 = warp_sums(c["mat"][0], c["abgd"][0], unit_plane(c, 0), *args)
    if not c["mode"]:
        return single(s0, bd, rbh), None
    conv = _rnd(s0, r1)
    s1 = warp_sums(c["mat"][1], c["abgd"][1], unit_plane(c, 1), *args)
    return average(conv, s1, bd, r0, r1, c["mode"] == 2, c["fwd"], c["bck"]), conv


# ---------------------------------------------------------------------------------------------
# batch records
# ---------------------------------------------------------------------------------------------
def ref_pictures(bd, w, h, n_refs, index):
    """The record's reference pictures: [reference][plane] arrays (uint8 at 8 bits, else uint16), no border."""
    sc = 1 << (bd - 8)
    out = []
    for r in range(n_refs):
        planes = []
        for p in range(3):
            pw, ph = w >> (p > 0), h >> (p > 0)
            y, x = np.mgrid[0:ph, 0:pw]
            d = draw(0x5750000000100000 + 256 * index + 4 * r + p, pw * ph, 64 * sc).reshape(ph, pw).astype(np.int64)
            planes.append(np.clip((2 * x + y) * sc // 4 + d, 0, (1 << bd) - 1).astype(np.uint16 if bd > 8 else np.uint8))
        out.append(planes)
    return out


def batch_cases():
    g = fixture()
    out = []
    for i in range(int(g["nbatch"][0])):
        bd, w, h, nr, chroma, nb, idx = [int(v) for v in g["q%d_par" % i][:7]]
        blocks = [dict(x=int(b[0]), y=int(b[1]), w=int(b[2]), h=int(b[3]), ref0=int(b[4]), ref1=int(b[5]), dist_wtd=int(b[6]),
                       fwd=int(b[7]), bck=int(b[8]), mat0=[int(v) for v in b[10:16]], mat1=[int(v) for v in b[16:22]])
                  for b in g["q%d_blocks" % i]]
        out.append(dict(name="q%d_bd%d_chroma%d" % (i, bd, chroma), bd=bd, w=w, h=h, n_refs=nr, chroma=chroma, index=idx, blocks=blocks,
                        kinds=g["q%d_kinds" % i], refs=ref_pictures(bd, w, h, nr, idx),
                        pred=[g["q%d_pred%d" % (i, p)] for p in range(3 if chroma else 1)]))
    return out


def block_planes(b, chroma):
    """The planes svtgpu_warp_predict_batch writes for block b: luma, and chroma from 16 x 16 up."""
    return (0, 1, 2) if chroma and b["w"] >= 16 and b["h"] >= 16 else (0,)


def predict_batch(refs, blocks, bd, w, h, chroma, fill=0):
    """What svt_aom_warped_motion_prediction writes for the blocks (no masked compound; blocks below 16 in a dimension luma
    only) into planes prefilled with `fill`."""
    dtype = refs[0][0].dtype
    pred = [np.full((h >> (p > 0), w >> (p > 0)), fill, dtype) for p in range(3)]
    for b in blocks:
        two = b["ref1"] != NO_REF
        r0, r1 = conv_rounds(bd, two)
        rbh = horiz_bits(bd, r0, bd > 8)
        for p in block_planes(b, chroma):
            ss = int(p > 0)
            x, y, bw, bh = b["x"] >> ss, b["y"] >> ss, b["w"] >> ss, b["h"] >> ss
            ok, abgd = shear_params(b["mat0"])
            assert ok == 1
            s0 = warp_sums(b["mat0"], abgd, refs[b["ref0"]][p], x, y, bw, bh, ss, ss, bd, rbh)
            if not two:
                v = single(s0, bd, rbh)
            else:
                ok, abgd1 = shear_params(b["mat1"])
                assert ok == 1
                s1 = warp_sums(b["mat1"], abgd1, refs[b["ref1"]][p], x, y, bw, bh, ss, ss, bd, rbh)
                v = average(_rnd(s0, r1), s1, bd, r0, r1, b["dist_wtd"], b["fwd"], b["bck"])
            pred[p][y:y + bh, x:x + bw] = v.astype(dtype)
    return pred


def expected_planes(c, blocks, fill):
    """The record's predictor samples of `blocks` over planes of `fill`: what a call on those blocks must leave."""
    dtype = c["refs"][0][0].dtype
    want = [np.full((c["h"] >> (p > 0), c["w"] >> (p > 0)), fill, dtype) for p in range(3)]
    for b in blocks:
        for p in block_planes(b, c["chroma"]):
            ss = int(p > 0)
            x, y, bw, bh = b["x"] >> ss, b["y"] >> ss, b["w"] >> ss, b["h"] >> ss
            want[p][y:y + bh, x:x + bw] = c["pred"][p][y:y + bh, x:x + bw]
    return want
