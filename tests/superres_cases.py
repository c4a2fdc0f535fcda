"""The super-resolution fixture tests/golden/superres.bin (the reference's own C through tests/golden/gen_golden_superres.c)
and a numpy restatement of the normative upscale (svt_av1_upscale_normative_rows, EbSuperRes.c:214-284), used as the
checker of the GPU tests where the fixture has no record (wider strides, the columns past the upscaled width)."""
import functools
import os

import numpy as np

import golden_io
import lr_cases as lc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superres.bin")
DENOMS = list(range(8, 18))


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN)


def scaled_size(dim, denom):
    """calculate_scaled_size_helper (EbSuperRes.c:22-41)."""
    if denom != 8 and denom <= 16:
        return max((dim * 8 + denom // 2) // denom, min(16, dim))
    if denom == 17:
        return (3 + dim * 3) >> 2
    return dim


def _cdiv(a, b):
    """C's integer division (truncation towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def geometry(in_w, out_w):
    """(x_step_qn, x0_qn): av1_get_upscale_convolve_step / get_upscale_convolve_x0 (EbSuperRes.c:43-52)."""
    step = ((in_w << 14) + out_w // 2) // out_w
    err = out_w * step - (in_w << 14)
    x0 = _cdiv(-((out_w - in_w) << 13) + out_w // 2, out_w) + 128 - _cdiv(err, 2)
    return step, x0 & 0x3fff


def upscale_plane(src, in_w, out_w, bd, dst_w=None, clip=True):
    """One plane: `src` is [rows][coded plane width]; source indices are clamped to the coded width.  Returns
    [rows][dst_w or out_w]: the columns at and past out_w repeat the row's last upscaled sample.  clip=False: the
    rounded sums before the clip (int64)."""
    filt = fixture()["filter"].astype(np.int64)
    step, x0 = geometry(in_w, out_w)
    dst_w = out_w if dst_w is None else dst_w
    xq = x0 + np.minimum(np.arange(dst_w), out_w - 1).astype(np.int64) * step
    idx = np.clip((xq >> 14)[:, None] - 4 + np.arange(8)[None, :], 0, src.shape[1] - 1)
    taps = filt[(xq & 0x3fff) >> 8]                       # [dst_w][8]
    s = (src.astype(np.int64)[:, idx] * taps[None]).sum(axis=2)
    s = (s + 64) >> 7
    return np.clip(s, 0, (1 << bd) - 1).astype(src.dtype) if clip else s


def upscale_frame(planes, frame_width, upscaled_width, bd, dst_widths=None):
    """svt_av1_superres_upscale_frame: three planes of a 4:2:0 picture, chroma widths rounded up."""
    out = []
    for p, a in enumerate(planes):
        sx = 1 if p else 0
        coded = ((frame_width + 7) & ~7) >> sx
        out.append(upscale_plane(a[:, :coded], (frame_width + sx) >> sx, (upscaled_width + sx) >> sx, bd,
                                 None if dst_widths is None else dst_widths[p]))
    return out


def up_cases():
    g = fixture()
    for i in range(int(g["nup"][0])):
        bd, sub_x, fw, uw, denom, rows, in_w, out_w, coded, ntile = (int(v) for v in g["up%d_par" % i])
        dt = np.uint16 if bd > 8 else np.uint8
        yield {"name": "up%d_%dto%d_bd%d_sx%d" % (i, fw, uw, bd, sub_x), "bd": bd, "sub_x": sub_x, "frame_width": fw,
               "upscaled_width": uw, "denom": denom, "rows": rows, "in_w": in_w, "out_w": out_w, "coded": coded,
               "ntile": ntile, "src": g["up%d_src" % i].astype(dt), "out": g["up%d_out" % i].astype(dt)}


def lr_cases():
    g = fixture()
    for i in range(int(g["nlr"][0])):
        w, h, bd, usize, mask, fw, denom = (int(v) for v in g["lr%d_params" % i])
        dt = np.uint16 if bd > 8 else np.uint8
        yield {"name": "lr%d_%dto%dx%d_bd%d" % (i, fw, w, h, bd), "w": w, "h": h, "bd": bd, "frame_width": fw,
               "denom": denom, "unit_size": [usize, usize >> 1, usize >> 1],
               "frame_type": [1 if mask >> p & 1 else 0 for p in range(3)],
               "units": [lc.rest_units_from_rows(g["lr%d_units%d" % (i, p)]) for p in range(3)],
               "dlf": [g["lr%d_dlf%d" % (i, p)].astype(dt) for p in range(3)],
               "cdef": [g["lr%d_cdef%d" % (i, p)].astype(dt) for p in range(3)],
               "out": [g["lr%d_out%d" % (i, p)].astype(dt) for p in range(3)]}
