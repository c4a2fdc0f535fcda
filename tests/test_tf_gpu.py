"""The temporal filter's filter half on the MI355X: the noise estimate (plain entry, both exported shims, the
asynchronous form), the seven plain-C library shims against every block / central / final record, and
svtgpu_tf_filter_frame against every frame record of the reference's fixture (tests/golden/tf.bin) and, on a frame the
fixture does not hold, against the numpy restatement that tests/test_tf.py holds to those records.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import svtgpu
import tf_cases as tc

pytestmark = pytest.mark.gpu

NOISE = list(tc.noise_cases())
BLOCKS = list(tc.block_cases())
CENTRAL = list(tc.central_cases())
FINAL = list(tc.final_cases())
FRAMES = list(tc.frame_cases())
_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _dev(a):
    """A device copy of a uint8 / uint16 array (torch has no uint16 arithmetic: the bits travel as int16)."""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


# ---------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(NOISE)))
def test_noise_matches_records(ctx, i):
    c = NOISE[i]
    stride = c["w"] + 5  # rows need no alignment
    buf = np.full((c["h"], stride), 3, c["src"].dtype)
    buf[:, :c["w"]] = c["src"]
    d = _dev(buf)
    assert svtgpu.tf_estimate_noise(ctx, d.data_ptr(), c["bd"], stride, c["w"], c["h"]) == c["out"], c["name"]


@pytest.mark.parametrize("i", range(len(NOISE)))
def test_noise_shims_match_records(i):
    c = NOISE[i]
    src = np.ascontiguousarray(c["src"])
    L = svtgpu.lib()
    if c["bd"] == 8:
        got = L.svtgpu_estimate_noise_fp16(svtgpu.ptr(src), c["w"], c["h"], c["w"])
    else:
        got = L.svtgpu_estimate_noise_highbd_fp16(svtgpu.ptr(src), c["w"], c["h"], c["w"], c["bd"])
    assert got == c["out"], c["name"]


def test_noise_async_then_read(ctx):
    """Two estimates queued back to back on one state: each read returns its own plane's value (the slot resets)."""
    st = svtgpu.TfState(ctx, 64, 48)
    for c in (NOISE[0], NOISE[-1], NOISE[1]):
        d = _dev(c["src"])
        st.estimate_noise_async(d.data_ptr(), c["bd"], c["w"], c["w"], c["h"])
        assert st.read_noise() == c["out"], c["name"]
    st.close()


# ---------------------------------------------------------------------------------------------
# the seven shims
# ---------------------------------------------------------------------------------------------
def _strided(planes, stride):
    """Each [h][w] plane inside rows of `stride` samples; returns the buffers."""
    out = []
    for p in planes:
        b = np.zeros((p.shape[0], stride), p.dtype)
        b[:, :p.shape[1]] = p
        out.append(b)
    return out


@pytest.mark.parametrize("i", range(len(BLOCKS)))
def test_block_shims_match_records(i):
    c = BLOCKS[i]
    L = svtgpu.lib()
    m = c["meta"]
    blk = svtgpu.TfBlock.make(m["split"], m["mv32"], m["mv16"], m["err32"], m["err16"])
    prm = svtgpu.TfParams.make(c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"], c["zz"])
    ss, ps = 72, 40  # source and predictor strides differ; accum / count follow the predictor's
    src, pre = _strided(c["src"], ss), _strided(c["pre"], ps)
    acc, cnt = _strided(c["accum_in"], ps), _strided(c["count_in"], ps)
    for a in acc + cnt:  # beyond the block: must stay as it is
        a[:, c["bw"]:] = 7
    pp = svtgpu.ptr
    tail = [c["bw"], c["bw"], 1, 1, pp(acc[0]), pp(cnt[0]), pp(acc[1]), pp(cnt[1]), pp(acc[2]), pp(cnt[2])]
    head = [ctypes.byref(blk), c["idx"], ctypes.byref(prm)]
    if c["zz"]:
        args = head + [pp(pre[0]), ps, pp(pre[1]), pp(pre[2]), ps] + tail
        fn = L.svtgpu_tf_apply_zz_planewise_medium if c["bd"] == 8 else L.svtgpu_tf_apply_zz_planewise_medium_hbd
    else:
        args = head + [pp(src[0]), ss, pp(pre[0]), ps, pp(src[1]), pp(src[2]), ss, pp(pre[1]), pp(pre[2]), ps] + tail
        fn = L.svtgpu_tf_apply_planewise_medium if c["bd"] == 8 else L.svtgpu_tf_apply_planewise_medium_hbd
    fn(*(args + ([c["bd"]] if c["bd"] > 8 else [])))
    for p in range(3):
        w = c["bw"] >> (p > 0)
        np.testing.assert_array_equal(acc[p][:, :w], c["accum"][p], err_msg="%s accum %d" % (c["name"], p))
        np.testing.assert_array_equal(cnt[p][:, :w], c["count"][p], err_msg="%s count %d" % (c["name"], p))
        assert (acc[p][:, c["bw"]:] == 7).all() and (cnt[p][:, c["bw"]:] == 7).all(), c["name"]


def _ptr_array(arrs):
    return (_P * 3)(*[a.ctypes.data for a in arrs])


@pytest.mark.parametrize("i", range(len(CENTRAL)))
def test_central_shims_match_records(i):
    c = CENTRAL[i]
    L = svtgpu.lib()
    src = [_strided([c["src"][p]], tc.CS >> (p > 0))[0] for p in range(3)]
    acc = [np.zeros(a.shape, np.uint32) for a in c["accum"]]
    cnt = [np.zeros(a.shape, np.uint16) for a in c["count"]]
    fn = L.svtgpu_tf_apply_filtering_central if c["bd"] == 8 else L.svtgpu_tf_apply_filtering_central_highbd
    fn(c["tf_chroma"], tc.CS, _ptr_array(src), _ptr_array(acc), _ptr_array(cnt), 64, 64, 1, 1)
    for p in range(3):
        np.testing.assert_array_equal(acc[p], c["accum"][p], err_msg="%s accum %d" % (c["name"], p))
        np.testing.assert_array_equal(cnt[p], c["count"][p], err_msg="%s count %d" % (c["name"], p))


@pytest.mark.parametrize("i", range(len(FINAL)))
def test_final_shim_matches_records(i):
    c = FINAL[i]
    dt = tc.dtype_of(c["bd"])
    out = [np.full((72, tc.CS >> (p > 0)), 9, dt) for p in range(3)]
    acc = [np.ascontiguousarray(a) for a in c["accum"]]
    cnt = [np.ascontiguousarray(a) for a in c["count"]]
    stride = (ctypes.c_uint32 * 3)(tc.CS, tc.CS // 2, tc.CS // 2)
    o8, o16 = (_ptr_array(out), None) if c["bd"] == 8 else (None, _ptr_array(out))
    svtgpu.lib().svtgpu_tf_get_final_filtered_pixels(1, o8, o16, _ptr_array(acc), _ptr_array(cnt), stride, 4 * tc.CS + 8,
                                                     2 * (tc.CS // 2) + 4, 32, 32, int(c["bd"] > 8))
    for p in range(3):
        w, y0, x0 = 64 >> (p > 0), 2 if p else 4, 4 if p else 8
        np.testing.assert_array_equal(out[p][y0:y0 + w, x0:x0 + w], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
        out[p][y0:y0 + w, x0:x0 + w] = 9
        assert (out[p] == 9).all(), c["name"]  # nothing but the block was written


# ---------------------------------------------------------------------------------------------
# whole pictures
# ---------------------------------------------------------------------------------------------
def _blocks(metas):
    return [svtgpu.TfBlock.make(m["split"], m["mv32"], m["mv16"], m["err32"], m["err16"]) for row in metas for m in row]


def _planes(tensors, arrays):
    return svtgpu.TfPlanes.make([t.data_ptr() for t in tensors], [a.shape[1] for a in arrays])


def _filter(state, centre, refs, metas, decay, mv_dist_th, tf_chroma, bd, zz, stream=None):
    """svtgpu_tf_filter_frame of planes given over the aligned area; returns the three output planes (aligned area)."""
    dc = [_dev(a) for a in centre]
    dr = [[_dev(a) for a in r] for r in refs]
    do = [_dev(np.full(a.shape, 5, a.dtype)) for a in centre]
    prm = svtgpu.TfParams.make(decay, mv_dist_th, tf_chroma, bd, zz)
    state.filter_frame(_planes(dc, centre), [_planes(t, r) for t, r in zip(dr, refs)], _blocks(metas), prm,
                       _planes(do, centre), stream)
    state.ctx.synchronize(stream)
    return [_host(t, a.dtype) for t, a in zip(do, centre)]


def _check_frame(c, got):
    for p in range(3):
        h, w = c["out"][p].shape
        np.testing.assert_array_equal(got[p][:h, :w], c["out"][p], err_msg="%s plane %d" % (c["name"], p))


@pytest.mark.parametrize("i", range(len(FRAMES)))
def test_frame_matches_records(ctx, i):
    c = FRAMES[i]
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _filter(st, c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"], c["zz"])
    _check_frame(c, got)
    if not c["tf_chroma"]:
        for p in (1, 2):
            np.testing.assert_array_equal(got[p], c["centre"][p], err_msg=c["name"])
    st.close()


def test_frame_on_a_created_stream(ctx):
    c = next(f for f in FRAMES if f["n_refs"] == 5 and f["bd"] == 10 and not f["zz"])
    s = ctx.stream_create()
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _filter(st, c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], c["tf_chroma"], c["bd"], c["zz"], s)
    _check_frame(c, got)
    st.close()
    ctx.stream_destroy(s)


def test_one_state_twice_with_other_reference_counts(ctx):
    """5 references, then 1, then 0 on one state: no metadata of an earlier call survives."""
    cs = [next(f for f in FRAMES if f["bd"] == 8 and f["n_refs"] == n and f["tf_chroma"]) for n in (5, 1, 0)]
    st = svtgpu.TfState(ctx, cs[0]["w"], cs[0]["h"])
    for c in cs:
        _check_frame(c, _filter(st, c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], c["tf_chroma"],
                                c["bd"], c["zz"]))
    st.close()


def cross_check_case():
    """200x136 10-bit, three references of growing error (the first equals the centre and has small block errors), so
    that the restatement meets a quadrant of weight 1000, one at the 112 clamp and one strictly between."""
    w, h, bd, aw, ah = 200, 136, 10, 256, 192
    rng = np.random.default_rng(7)
    centre = [rng.integers(0, 1024, (ah >> (p > 0), aw >> (p > 0))).astype(np.uint16) for p in range(3)]
    refs = []
    for amp in (0, 24, 300):
        refs.append([np.clip(c.astype(np.int64) + rng.integers(-amp, amp + 1, c.shape), 0, 1023).astype(np.uint16)
                     for c in centre])
    metas = tc.random_metas(rng, 3, 12, bd)
    for m in metas[0]:
        m["err32"] //= np.uint64(200)
        m["err16"] //= np.uint64(200)
    return dict(w=w, h=h, bd=bd, centre=centre, refs=refs, metas=metas, decay=[6000000, 9000000, 12000000], mv_dist_th=1080)


def test_frame_cross_check_against_the_restatement(ctx):
    c = cross_check_case()
    stats = []
    want = tc.filter_frame(c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], 1, c["bd"], 0, c["w"], c["h"], stats)
    assert any(sd == 112 for sd, _, _ in stats) and any(wt == 1000 for _, wt, _ in stats)
    assert any(0 < sd < 112 for sd, _, _ in stats)
    st = svtgpu.TfState(ctx, c["w"], c["h"])
    got = _filter(st, c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], 1, c["bd"], 0)
    for p in range(3):
        hh, ww = c["h"] >> (p > 0), c["w"] >> (p > 0)
        np.testing.assert_array_equal(got[p][:hh, :ww], want[p][:hh, :ww], err_msg="plane %d" % p)
    st.close()
