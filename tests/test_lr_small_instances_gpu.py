"""Routing of the resident searches' items between their two instances, at the smallest frames in which each routing
case occurs.  Self-guided: sgr_res_kernel (every size, row parts) and sgr_res_small_kernel (one-part units of at most 10
chunks per pixel lane, 10 * 448 * 4 = 17 920 samples).  Wiener: wiener_res_kernel (every size) and
wiener_res_small_kernel (one-part units whose window fits 38 KB of LDS and whose rows fit 256 lanes x 32 rows).
Which instances ran is observed, not only predicted: the search's profiler counts the launches of each class (one per
instance with items), and each case asserts the count its routing implies.  The whole search (wn / sg level 1) against the CPU oracle, bit for
bit: frame types and every unit record, as test_lr_gpu.py compares them.  Each case asserts the unit grid it relies
on, computed here from AV1's unit-count rule, so a shape cannot silently stop exercising its case."""
import functools

import numpy as np
import pytest

import extreme_cases as ec
import oracle
import svtgpu
import synth

pytestmark = pytest.mark.gpu

SR_PL, SR_KMAX, SRS_KMAX = 448, 19, 10  # pixel lanes per workgroup; chunks per lane of the big / small instance


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _count(unit, extent):
    """av1_lr_count_units_in_tile: units of `unit` samples over `extent`, the last one taking the remainder."""
    return max((extent + (unit >> 1)) // unit, 1)


def _grid(unit, w, h, chroma=False):
    """The (w, h) of every unit of a plane.  Unit rows start RESTORATION_UNIT_OFFSET (8 luma rows) above the multiples
    of the unit size: the first row of several is that much shorter, the last takes the remainder."""
    nx, ny = _count(unit, w), _count(unit, h)
    off = 8 >> (1 if chroma else 0)
    ws = [unit] * (nx - 1) + [w - unit * (nx - 1)]
    ys = [0] + [r * unit - off for r in range(1, ny)] + [h]
    return [(uw, ys[r + 1] - ys[r]) for r in range(ny) for uw in ws]


def _route(uw, uh):
    """'small', 'big' (one part) or 'parted' for a unit, by the planner's rule."""
    chunks = ((uw + 3) >> 2) * uh
    k = -(-chunks // SR_PL)
    if k > SR_KMAX:
        return "parted"
    return "small" if k <= SRS_KMAX else "big"


WR_NT, WR_RMAX, WRS_NT, WRS_RMAX, WRS_LDS_CAP = 1024, 32, 256, 32, 38 * 1024


def _wr_route(uw, uh):
    """'small' or 'big' for a unit's Wiener descent, by the planner's rule."""
    cpw = (((uw + 1) >> 1) + 63) & ~63
    nseg = WRS_NT // cpw
    window = (uh + 6) * ((uw + 10) >> 1) * 4
    return "small" if nseg > 0 and -(-uh // nseg) <= WRS_RMAX and window <= WRS_LDS_CAP else "big"


def _launches(w, h, unit_size):
    """(Wiener descent launches, self-guided search launches) of a frame: one per instance that has a unit."""
    units = [u for p in range(3) for u in _grid(unit_size[p], w if p == 0 else (w + 1) // 2, h if p == 0 else (h + 1) // 2,
                                                p > 0)]
    return (len(set(_wr_route(*u) for u in units)), len(set(_route(*u) == "small" for u in units)))


def _routes(w, h, unit_size):
    return [sorted(set(_route(*u) for u in _grid(unit_size[p], w if p == 0 else (w + 1) // 2,
                                                   h if p == 0 else (h + 1) // 2, p > 0))) for p in range(3)]


def _crop_pair(w, h, bd, seed):
    src, rec = synth.frame_pair((w + 7) & ~7, (h + 7) & ~7, bd, seed=seed)
    cut = lambda planes: [np.ascontiguousarray(a[:(h if p == 0 else (h + 1) // 2), :(w if p == 0 else (w + 1) // 2)])
                          for p, a in enumerate(planes)]
    return cut(src), cut(rec)


def _coded(planes, seed):
    """Crop-size planes inside the 8-aligned coded frame, random past the crop (a read of them would show)."""
    h, w = planes[0].shape
    w8, h8 = (w + 7) & ~7, (h + 7) & ~7
    if (w8, h8) == (w, h):
        return planes
    r = np.random.default_rng(seed)
    out = []
    for p, a in enumerate(planes):
        pw, ph = (w8, h8) if p == 0 else (w8 // 2, h8 // 2)
        b = r.integers(0, int(a.max()) + 1, (ph, pw)).astype(a.dtype)
        b[:a.shape[0], :a.shape[1]] = a
        out.append(b)
    return out


def _ctrls(mod):
    return mod.lr_controls(1, 1, rdmult=7000, switchable=(300, 700, 900), wiener=(250, 800), sgrproj=(250, 900))


# name: (w, h, bd, unit sizes, the routes of (luma, chroma) units)
SHAPES = {
    # luma one 320 x 200 unit in row parts on the big kernel; chroma one 160 x 100 unit (K = 9) on the small one
    "mixed": (320, 200, 10, [256, 128, 128], (["parted"], ["small"])),
    # chroma width 165: 42 chunk columns, the last one of a single sample (the small instance's last-column masks)
    "odd": (330, 182, 8, [256, 128, 128], (["parted"], ["small"])),
    # chroma units 128 x 184 (K = 14): over the small capacity, unparted on the big kernel beside the parted luma
    "tall": (512, 368, 10, [256, 128, 128], (["parted"], ["big"])),
    # every unit 128 wide: luma 128 x 120 and 128 x 136 (K = 10 = the small capacity exactly), chroma 128 x 128 -- only
    # the small self-guided instance launches; the 136-row units exceed the small Wiener instance's 32 rows per segment
    "all_small": (256, 256, 10, [128, 128, 128], (["small"], ["small"])),
    # luma two 256 x 256 units (two self-guided row parts each; the big Wiener instance), chroma two 128 x 128 units on
    # both small instances: both Wiener instances launch
    "wn_mixed": (512, 256, 10, [256, 128, 128], (["parted"], ["small"])),
}
# (Wiener descent launches, self-guided search launches) each shape must show
LAUNCHES = {"mixed": (1, 2), "odd": (1, 2), "tall": (1, 1), "all_small": (2, 1), "wn_mixed": (2, 2)}


@functools.lru_cache(maxsize=None)
def _case(name, content=None):
    w, h, bd, us, _ = SHAPES[name]
    if content is None:
        src, rec = _crop_pair(w, h, bd, seed=0x5EED0B00 + w + h)
    else:
        rec, src = ec.planes(content[0], w, h, bd), ec.planes(content[1], w, h, bd)
    want = oracle.lr_search_frame(rec, src, bd, us, _ctrls(oracle))
    return rec, src, want


def _upload(ctx, rec, src, bd):
    rec8, src8 = _coded(rec, 3), _coded(src, 4)
    R, S = (svtgpu.Frame(ctx, rec8[0].shape[1], rec8[0].shape[0], bd) for _ in range(2))
    R.upload(rec8)
    S.upload(src8)
    return R, S


def _check(ctx, name, content=None):
    w, h, bd, us, _ = SHAPES[name]
    rec, src, (want_ft, want_units, want_recs) = _case(name, content)
    R, S = _upload(ctx, rec, src, bd)
    st = svtgpu.LrState(ctx, w, h, us)
    st.profile(True)
    ft, recs = st.search(R, S, _ctrls(svtgpu), records=True)
    prof = st.profile(False)
    # the instances that ran: one launch of the class per instance with items
    assert (prof["wiener_trials"]["launches"], prof["projection"]["launches"]) == LAUNCHES[name], (name, prof)
    assert ft == want_ft
    for p in range(3):
        np.testing.assert_array_equal(recs[p]["sse"], want_recs[p]["sse"], err_msg="plane %d sse" % p)
        np.testing.assert_array_equal(recs[p]["sgrproj"], want_recs[p]["sgrproj"], err_msg="plane %d sgrproj" % p)
        ok = recs[p]["sse"][:, 1] != np.iinfo(np.int64).max
        np.testing.assert_array_equal(recs[p]["wiener"][ok], want_recs[p]["wiener"][ok], err_msg="plane %d" % p)
    st.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_unit_grid_exercises_its_routing_case(name):
    w, h, bd, us, (luma, chroma) = SHAPES[name]
    assert _routes(w, h, us) == [luma, chroma, chroma]
    assert _launches(w, h, us) == LAUNCHES[name]
    if name == "odd":
        assert ((w + 1) // 2) % 4 == 1
    if name == "all_small":  # at the capacity boundary, not below it
        assert max(-(-((uw + 3) >> 2) * uh // SR_PL) for uw, uh in _grid(us[0], w, h)) == SRS_KMAX


@pytest.mark.parametrize("name", list(SHAPES))
def test_search_vs_oracle(ctx, name):
    _check(ctx, name)


# checkerboard against all-maximum and the reverse: |x - src| = maxv on every other sample, the filters' g and the
# candidate errors of the small instance's passes at their bounds
@pytest.mark.parametrize("content", [("checker", "max"), ("max", "checker"), ("checker", "anti")])
def test_search_extreme_content_vs_oracle(ctx, content):
    _check(ctx, "mixed", content)


def test_async_search_on_the_mixed_shape(ctx):
    """svtgpu_lr_search_frame_async + the device finish: the reference's frame types, and the frame restored from the
    units it left on the device equals the one restored from the synchronous search's."""
    w, h, bd, us, _ = SHAPES["mixed"]
    rec, src, (want_ft, _, _) = _case("mixed")
    R, S = _upload(ctx, rec, src, bd)
    D, O1, O2 = (svtgpu.Frame(ctx, R.width, R.height, bd) for _ in range(3))
    D.upload(_coded(rec, 3))
    st = svtgpu.LrState(ctx, w, h, us)
    ft = st.search(R, S, _ctrls(svtgpu))
    ft = ft[0] if isinstance(ft, tuple) else ft
    st.apply(D, R, O1, ft)
    st2 = svtgpu.LrState(ctx, w, h, us)
    st2.search_async(R, S, _ctrls(svtgpu))
    st2.apply(D, R, O2, None)
    assert st2.read_result() == ft == want_ft
    for a, b in zip(O1.download(), O2.download()):
        assert np.array_equal(a, b)
    st.close()
    st2.close()
