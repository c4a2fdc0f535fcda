"""The self-guided filter planes of every searched ep (sgr_flt_kernel), read back with svtgpu_lr_read_sgr_planes and
compared sample by sample with the CPU oracle: the search's records only show the winning ep's SSE, so a wrong sample
of a losing ep would pass them."""
import numpy as np
import pytest

import oracle
import svtgpu
import synth

pytestmark = pytest.mark.gpu

SGR_R = [(2, 1)] * 10 + [(0, 1)] * 4 + [(2, 0)] * 2  # radii of the 16 parameter sets (r = 2 pass, r = 1 pass)


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _crop(planes, w, h):
    return [np.ascontiguousarray(a[:(h if p == 0 else (h + 1) // 2), :(w if p == 0 else (w + 1) // 2)])
            for p, a in enumerate(planes)]


def _coded(planes, bd, seed):
    """The crop-size planes inside the 8-aligned coded frame, random past the crop (a read of it would show)."""
    h, w = planes[0].shape
    w8, h8 = (w + 7) & ~7, (h + 7) & ~7
    r = np.random.default_rng(seed)
    out = []
    for p, a in enumerate(planes):
        b = r.integers(0, 1 << bd, ((h8, w8) if p == 0 else (h8 // 2, w8 // 2))).astype(a.dtype)
        b[:a.shape[0], :a.shape[1]] = a
        out.append(b)
    return out


def _data(kind, w, h, bd, seed):
    w8, h8 = (w + 7) & ~7, (h + 7) & ~7
    src, rec = synth.frame_pair_int(w8, h8, bd, seed)
    if kind != "int":
        mx = (1 << bd) - 1
        for a in rec:
            if kind == "max":
                a[...] = mx
            else:  # max / 0 checkerboard: the largest variance, p * s at its wrap and clamp range, z = 255
                yy, xx = np.indices(a.shape)
                a[...] = np.where((yy + xx) & 1, mx, 0)
    return _crop(src, w, h), _crop(rec, w, h)


def _check_planes(ctx, w, h, bd, kind, seed):
    src, rec = _data(kind, w, h, bd, seed)
    R, S = (svtgpu.Frame(ctx, (w + 7) & ~7, (h + 7) & ~7, bd) for _ in range(2))
    R.upload(_coded(rec, bd, 3))
    S.upload(_coded(src, bd, 4))
    st = svtgpu.LrState(ctx, w, h, [64, 32, 32])
    st.search(R, S, svtgpu.lr_controls(1, 1, rdmult=7000, switchable=(300, 700, 900), wiener=(250, 800),
                                       sgrproj=(250, 900)))
    for p in range(3):
        ph, pw = rec[p].shape
        dgd = rec[p].astype(np.int32)
        pad = np.pad(dgd, 3, mode="edge")  # the search runs without stripe boundaries: the edge-clamped plane
        for slot in range(16):  # sg level 1 searches all 16 parameter sets, slot == ep
            ep, f0, f1 = st.read_sgr_planes(p, slot)
            assert ep == slot
            w0, w1 = oracle.sgr_filter(pad, pw, ph, ep, bd)
            for r, got, want in ((SGR_R[ep][0], f0, w0), (SGR_R[ep][1], f1, w1)):
                assert (got is not None) == (r > 0), (p, ep)
                if r:
                    g = (want - (dgd << 4)).astype(np.int16)
                    bad = np.argwhere(got != g)
                    assert bad.size == 0, "plane %d ep %d r %d: %d samples differ, first at %s" % (
                        p, ep, r, len(bad), bad[0])
    st.close()


# 330x182: luma tiles 64 .. 10 wide and a partial tile height, chroma 165x91 (odd width: the unpaired last column; odd
# height: the last row pair's missing second row).  134x70: 6-wide and 6-high last tiles, chroma 67x35.  128x128: only
# full 64x64 luma tiles, with neighbours on every side of the inner tile boundaries.  66x8: the lowest frame the library
# accepts (svtgpu_lr_state_create refuses a height below 8), so the chroma planes are 4 rows high, not fewer
SHAPES = [(330, 182, 8), (134, 70, 10), (128, 128, 10), (66, 8, 10)]


@pytest.mark.parametrize("w,h,bd", SHAPES)
def test_sgr_flt_planes_every_ep(ctx, w, h, bd):
    """Every sample of both filter planes of all 16 eps equals oracle.sgr_filter(...) - (dgd << 4) as int16; the slots
    that share an r = 1 plane (eps 2/11, 5/12, 8/13: equal s) read the same data.  The lowest case is 66x8 (chroma 33x4):
    the library accepts no frame lower than 8 rows."""
    _check_planes(ctx, w, h, bd, "int", 0x5EED0A00 + w)


@pytest.mark.parametrize("kind", ["max", "checker"])
@pytest.mark.parametrize("w,h,bd", [(134, 70, 10), (330, 182, 8)])
def test_sgr_flt_planes_extreme_samples(ctx, w, h, bd, kind):
    """All samples at the bit-depth maximum (the largest box sums, p = 0) and a max / 0 checkerboard (the largest
    p: p * s wraps as the reference's u32 product does and z clamps at 255)."""
    _check_planes(ctx, w, h, bd, kind, 0x5EED0B00 + w)
