"""Edge cases of the fused CDEF strength search (csrc/cdef_search.hip) against the CPU oracle, bit for bit.

The kernel zeroes a lane that is not measured once (sample, clamp range, taps, secondary sums) instead of masking its
output per strength, keeps 16 x + 8 per sample for the rounding, and forms the luma squared error from sum d^2,
sum d s and sum s^2.  Each case below is the smallest frame at which one of those can go wrong; every case runs at
8 and at 10 bit.  `mse` and `skip` are compared for every searched filter block, `dir` and `var` for its listed blocks
(what test_cdef_frame_pipeline_vs_oracle compares)."""
import functools

import numpy as np
import pytest

import oracle
import svtgpu
import synth


def _noise_src(w, h, bd, seed):
    return synth.frame_pair(w, h, bd, seed)[0]


def _planes(w, h, bd, fill):
    dt = np.uint16 if bd > 8 else np.uint8
    return [np.full((h, w) if p == 0 else (h // 2, w // 2), fill, dt) for p in range(3)]


def _pair_mask():
    """64x64: rows 2 and 5 of 8x8 blocks skipped whole; in rows 0 and 1 exactly one block of every horizontal pair
    (the two 4x4 chroma blocks of one 8-sample chroma segment) is skipped, the left one in row 0, the right in row 1."""
    m = np.ones((8, 8), np.uint8)
    m[2, :] = 0
    m[5, :] = 0
    m[0, 0::2] = 0
    m[1, 1::2] = 0
    m[6, 3] = 0
    return m


def _isolated(bd):
    """Flat field with isolated dark and bright samples (negative and positive tap sums; bright ones next to the
    picture edge put the apron beside the clamp range's maximum)."""
    top = (1 << bd) - 1
    rec = _planes(64, 64, bd, top // 2)
    rng = np.random.Generator(np.random.PCG64(0xCDEF + bd))
    for p in rec:
        n = p.shape[0]
        ys, xs = rng.integers(0, n, 40), rng.integers(0, n, 40)
        p[ys[:20], xs[:20]] = rng.integers(0, top // 8, 20)
        p[ys[20:], xs[20:]] = top - rng.integers(0, top // 8, 20)
        p[0, 0], p[0, n - 1], p[n - 1, 0], p[n - 1, n - 1] = top, 0, 0, top
        p[1, 5], p[5, 1], p[n - 2, 9] = 0, top, top
    return rec


def _checker(bd):
    top = (1 << bd) - 1
    rec = _planes(64, 64, bd, 0)
    for p in rec:
        yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
        p[(yy + xx) % 2 == 1] = top
    return rec


# name -> (w, h, cdef_level, q, mask builder or None, recon builder or None (synthetic pair), fb_bsize or None)
CASES = {
    "72x72": (72, 72, 1, 128, None, None, None),
    "64x64_pairmask": (64, 64, 1, 140, _pair_mask, None, None),
    "128x64_level9": (128, 64, 9, 255, None, None, None),
    "128x64_level2": (128, 64, 2, 60, None, None, None),
    "64x64_isolated": (64, 64, 1, 128, None, _isolated, None),
    "64x64_checker": (64, 64, 1, 128, None, _checker, None),
    "64x64_flat": (64, 64, 1, 128, None, lambda bd: _planes(64, 64, bd, 100 << (bd - 8)), None),
    "128x128_sb128": (128, 128, 1, 140, None, None, [15, 15, 15, 15]),  # BLOCK_128X128 at every filter block
}
PARAMS = [(n, bd) for n in CASES for bd in (8, 10)]


@functools.lru_cache(maxsize=None)
def _case(name, bd):
    """(src, rec, mask, fb_bsize, ctrls args, oracle result): built once, shared by the CPU and GPU tests, never
    written to."""
    w, h, level, q, mk, rk, fbb = CASES[name]
    seed = 0x5EED0800 + w + 3 * h + bd + level
    if rk is None:
        src, rec = synth.frame_pair(w, h, bd, seed)
    else:
        src, rec = _noise_src(w, h, bd, seed), rk(bd)
    mask = None if mk is None else mk()
    fbb = None if fbb is None else np.array(fbb, np.uint8)
    want = oracle.cdef_search_frame(rec, src, bd, svtgpu.cdef_controls(level), q, mask, fbb)
    for a in list(src) + list(rec) + list(want):
        a.setflags(write=False)
    return src, rec, mask, fbb, level, q, want


@pytest.mark.parametrize("name,bd", PARAMS)
def test_oracle_runs_every_case(name, bd):
    """CPU: the oracle evaluates the case and its mask leaves at least one filter block to search."""
    src, rec, mask, fbb, level, q, (omse, oskip, od, ov) = _case(name, bd)
    assert (oskip == 0).any()
    assert omse[:, oskip == 0].any()
    if name == "64x64_flat":  # nothing to filter: every searched strength measures the same picture
        live = omse[0, 0][omse[0, 0] != 0]
        assert live.size and np.unique(live).size == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,bd", PARAMS)
def test_cdef_search_edges_vs_oracle(name, bd):
    src, rec, mask, fbb, level, q, (omse, oskip, od, ov) = _case(name, bd)
    h, w = rec[0].shape
    ctx = svtgpu.Context(0)
    R, S = svtgpu.Frame(ctx, w, h, bd), svtgpu.Frame(ctx, w, h, bd)
    R.upload(rec)
    S.upload(src)
    st = svtgpu.CdefState(ctx, w, h)
    st.set_block_mask(mask)
    if fbb is not None:
        st.set_fb_bsize(fbb)
    st.search(R, S, svtgpu.cdef_controls(level), q)
    mse, skip, d, v = st.read()
    np.testing.assert_array_equal(skip, oskip)
    live = oskip == 0
    np.testing.assert_array_equal(mse[:, live], omse[:, live])
    nhfb = (w // 4 + 15) // 16
    lm = np.zeros_like(od, dtype=bool)
    for fb in np.nonzero(live)[0]:
        fbr, fbc = divmod(int(fb), nhfb)
        for b in range(64):
            r, c = 8 * fbr + b // 8, 8 * fbc + b % 8
            lm[fb, b] = 8 * r < h and 8 * c < w and (mask is None or mask[r, c])
    # the SB128 area's mse row (filter block 0, the only live one) is the fold of its four 64x64 parts' sums and
    # remainders (cdef_sb128.hip)
    np.testing.assert_array_equal(d[lm], od[lm])
    np.testing.assert_array_equal(v[lm], ov[lm])
    if name == "64x64_flat":
        vals = mse[0, 0][mse[0, 0] != 0]
        assert vals.size and np.unique(vals).size == 1
