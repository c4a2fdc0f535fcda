"""The frame-resizer fixture tests/golden/resize.bin (the reference's own C through tests/golden/gen_golden_resize.c) and a
numpy restatement of svt_av1_resize_plane_c / svt_av1_highbd_resize_plane_c (EbResize.c:148-737) with its tables taken
from the fixture, used as the checker of the GPU tests where the fixture has no record."""
import functools
import os

import numpy as np

import golden_io

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize.bin")
# the device kernels' tiles (csrc/resize.hip kTileW, kRowsPerWg): a wave makes TILE_W adjacent outputs of a row and a
# workgroup TILE_ROWS rows; the vertical kernels' workgroup makes TILE_ROWS output rows of TILE_W columns
TILE_W, TILE_ROWS = 512, 4


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN)


def _cdiv(a, b):
    """C's integer division (truncation towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def down2_steps(in_len, out_len):
    """get_down2_steps (EbResize.c:153-167)."""
    steps = 0
    while (in_len + 1) >> 1 >= out_len:
        steps += 1
        in_len = (in_len + 1) >> 1
        if in_len == 1:
            break
    return steps


def plan(in_len, out_len):
    """(halving steps, the length that reaches the interpolation, table index or -1, delta, offset) of one 1-D resize:
    resize_multistep, choose_interp_filter and the locals of svt_av1_interpolate_core_c (EbResize.c:265-387)."""
    if in_len == out_len:
        return 0, in_len, -1, 0, 0
    steps, n = down2_steps(in_len, out_len), in_len
    for _ in range(steps):
        n = (n + 1) >> 1
    if n == out_len:
        return steps, n, -1, 0, 0
    o16 = out_len * 16
    idx = 4 if o16 >= n * 16 else 3 if o16 >= n * 13 else 2 if o16 >= n * 11 else 1 if o16 >= n * 9 else 0
    delta = ((n << 14) + out_len // 2) // out_len
    half = (abs(n - out_len) << 13) + out_len // 2
    offset = half // out_len if n > out_len else _cdiv(-half, out_len)
    return steps, n, idx, delta, offset


def _taps8(a, pos, taps, maxv, clip=True):
    """Along the last axis of int64 `a`: output x is sum_k taps[x][k] * a[clamp((pos[x] >> 14) - 3 + k)], rounded by 7
    bits and clipped."""
    idx = np.clip((pos >> 14)[:, None] - 3 + np.arange(8)[None, :], 0, a.shape[-1] - 1)
    s = ((a[..., idx] * taps).sum(axis=-1) + 64) >> 7
    return np.clip(s, 0, maxv) if clip else s


def resize_1d(a, out_len, bd, clip_last=True):
    """resize_multistep of every row of int64 `a` (the last axis).  clip_last=False: the last stage's rounded sums
    before the clip."""
    g = fixture()
    maxv = (1 << bd) - 1
    steps, _, idx, delta, offset = plan(a.shape[-1], out_len)
    if a.shape[-1] == out_len:
        return a
    even, odd = (g["half_filters"][k].astype(np.int64) for k in range(2))
    for s in range(steps):
        n = a.shape[-1]
        # svt_av1_down2_symeven / down2_symodd as eight taps around 2 * i (the odd filter's eighth tap is 0)
        t = (np.concatenate([even[::-1], even]) if n % 2 == 0 else
             np.concatenate([odd[:0:-1], odd, [0]])).astype(np.int64)
        pos = (2 * np.arange((n + 1) >> 1, dtype=np.int64)) << 14
        a = _taps8(a, pos, t[None, :], maxv, clip_last or s < steps - 1 or idx >= 0)
    if idx >= 0:
        pos = offset + 128 + np.arange(out_len, dtype=np.int64) * delta
        a = _taps8(a, pos, g["filters"][idx].astype(np.int64)[(pos >> 8) & 63], maxv, clip_last)
    return a


def resize_plane(src, out_w, out_h, bd):
    """svt_av1_(highbd_)resize_plane_c: every row to out_w, clipped, then every column to out_h."""
    a = resize_1d(src.astype(np.int64), out_w, bd)
    a = resize_1d(np.ascontiguousarray(a.T), out_h, bd).T
    return np.ascontiguousarray(a).astype(src.dtype)


def resize_frame(planes, src_w, src_h, dst_w, dst_h, bd):
    """svt_aom_resize_frame (EbResize.c:887-973): the three 4:2:0 planes, chroma sizes (dim + 1) >> 1 on both sides."""
    out = []
    for p, a in enumerate(planes):
        s = 1 if p else 0
        out.append(resize_plane(a[:(src_h + s) >> s, :(src_w + s) >> s], (dst_w + s) >> s, (dst_h + s) >> s, bd))
    return out


def plane_cases():
    g = fixture()
    for i in range(int(g["nplane"][0])):
        bd, in_w, in_h, out_w, out_h, content = (int(v) for v in g["p%d_par" % i])
        yield {"name": "p%d_%dx%dto%dx%d_bd%d%s" % (i, in_w, in_h, out_w, out_h, bd, "_extreme" if content else ""),
               "index": i, "bd": bd, "in_w": in_w, "in_h": in_h, "out_w": out_w, "out_h": out_h, "content": content,
               "src": g["p%d_src" % i], "out": g["p%d_out" % i], "clipped": tuple(int(v) for v in g["clipped"][i])}


def frame_cases():
    g = fixture()
    for i in range(int(g["nframe"][0])):
        bd, sw, sh, dw, dh = (int(v) for v in g["f%d_par" % i])
        yield {"name": "f%d_%dx%dto%dx%d_bd%d" % (i, sw, sh, dw, dh, bd), "bd": bd, "src_w": sw, "src_h": sh,
               "dst_w": dw, "dst_h": dh, "src": [g["f%d_src%d" % (i, p)] for p in range(3)],
               "out": [g["f%d_out%d" % (i, p)] for p in range(3)]}
