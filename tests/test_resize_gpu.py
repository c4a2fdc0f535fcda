"""The frame resizer on the MI355X: svtgpu_resize_plane, svtgpu_resize_frame / svtgpu.resize() and the two RTCD shims
against every record of the reference's fixture (tests/golden/resize.bin), and against the numpy restatement that
tests/test_resize.py holds to those records where the fixture has none.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import resize_cases as rc
import svtgpu

pytestmark = pytest.mark.gpu

PLANES = list(rc.plane_cases())
FRAMES = list(rc.frame_cases())
SENTINEL = 0xA5
GUARD = 2  # sentinel rows above and below the destination


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


def _src_buffer(src, stride, shift, bd):
    """`src` laid out with `stride` samples per row from sample `shift` of a buffer; what lies between the rows is random."""
    r = np.random.default_rng(src.shape[1] * 131 + src.shape[0])
    buf = r.integers(0, 1 << bd, (src.shape[0] * stride + shift,)).astype(src.dtype)
    for y in range(src.shape[0]):
        buf[shift + y * stride:shift + y * stride + src.shape[1]] = src[y]
    return buf


def _enqueue(ctx, src, out_w, out_h, bd, src_stride, dst_stride, shift=0, stream=None):
    """Enqueues svtgpu_resize_plane; returns what the later check needs (the tensors stay alive in it)."""
    dt = src.dtype
    s = _dev(_src_buffer(src, src_stride, shift, bd))
    d = _dev(np.full(((out_h + 2 * GUARD) * dst_stride + shift,), SENTINEL, dt))
    rc_ = svtgpu.lib().svtgpu_resize_plane(s.data_ptr() + shift * dt.itemsize, dt.itemsize * 8, src_stride, src.shape[1],
                                           src.shape[0], d.data_ptr() + (shift + GUARD * dst_stride) * dt.itemsize,
                                           dst_stride, out_w, out_h, bd, stream if stream else ctx.stream)
    assert rc_ == 0, rc_
    return s, d, dt, shift, dst_stride, out_w, out_h


def _collect(job):
    """(the out_h x out_w samples written, True when every other sample of the destination buffer is untouched)."""
    s, d, dt, shift, dst_stride, out_w, out_h = job
    got = _host(d, dt)
    body = got[shift:].reshape(out_h + 2 * GUARD, dst_stride)
    out = body[GUARD:GUARD + out_h, :out_w].copy()
    body[GUARD:GUARD + out_h, :out_w] = SENTINEL
    return out, bool((got == SENTINEL).all())


def _plane(ctx, src, out_w, out_h, bd, src_extra=0, dst_extra=16, shift=0):
    job = _enqueue(ctx, src, out_w, out_h, bd, ((src.shape[1] + 15) & ~15) + src_extra, ((out_w + 15) & ~15) + dst_extra,
                   shift)
    ctx.synchronize()
    return _collect(job)


@pytest.mark.parametrize("i", range(len(PLANES)))
def test_plane_matches_records(ctx, i):
    c = PLANES[i]
    got, untouched = _plane(ctx, c["src"], c["out_w"], c["out_h"], c["bd"])
    np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])
    assert untouched, c["name"]  # the sentinel columns and rows around the destination


STRIDE_CASES = [i for i, c in enumerate(PLANES) if (c["in_w"], c["in_h"]) in ((88, 16), (83, 17), (100, 40), (5, 5))
                or c["out_w"] > rc.TILE_W or c["out_h"] > 500]


@pytest.mark.parametrize("i", STRIDE_CASES)
@pytest.mark.parametrize("src_extra,dst_extra,shift", [(16, 32, 0), (3, 5, 0), (21, 7, 5)])
def test_strides_and_alignment_do_not_matter(ctx, i, src_extra, dst_extra, shift):
    """Wider strides, rows that start at no 16-byte boundary (the one-sample loads and stores) and planes that start
    inside their buffers give the recorded output and write nothing else."""
    c = PLANES[i]
    got, untouched = _plane(ctx, c["src"], c["out_w"], c["out_h"], c["bd"], src_extra, dst_extra, shift)
    np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])
    assert untouched, c["name"]


def _frames(ctx, planes, sw, sh, dw, dh, bd, seed):
    """Device frames (sizes rounded up to 8) holding `planes` in their top-left corner, the rest random / a fill."""
    dt = np.uint16 if bd > 8 else np.uint8
    W, H, W2, H2 = (sw + 7) & ~7, (sh + 7) & ~7, (dw + 7) & ~7, (dh + 7) & ~7
    r = np.random.default_rng(seed)
    full = [r.integers(0, 1 << bd, (H >> (p > 0), W >> (p > 0))).astype(dt) for p in range(3)]
    for p in range(3):
        full[p][:planes[p].shape[0], :planes[p].shape[1]] = planes[p]
    fill = [np.full((H2 >> (p > 0), W2 >> (p > 0)), 0x55, dt) for p in range(3)]
    S, D = svtgpu.Frame(ctx, W, H, bd), svtgpu.Frame(ctx, W2, H2, bd)
    S.upload(full)
    D.upload(fill)
    return S, D, full


def _check_frame(D, want, name):
    got = D.download()
    for p in range(3):
        h, w = want[p].shape
        np.testing.assert_array_equal(got[p][:h, :w], want[p], err_msg="%s plane %d" % (name, p))
        rest = got[p].copy()
        rest[:h, :w] = 0x55
        assert (rest == 0x55).all(), "%s plane %d: samples outside the crop were written" % (name, p)


@pytest.mark.parametrize("i", range(len(FRAMES)))
@pytest.mark.parametrize("binding", ["c", "python"])
def test_frame_matches_records(ctx, i, binding):
    c = FRAMES[i]
    S, D, _ = _frames(ctx, c["src"], c["src_w"], c["src_h"], c["dst_w"], c["dst_h"], c["bd"], i)
    if binding == "c":
        assert svtgpu.lib().svtgpu_resize_frame(S.h, D.h, c["src_w"], c["src_h"], c["dst_w"], c["dst_h"], None) == 0
    else:
        svtgpu.resize(S, D, c["src_w"], c["src_h"], c["dst_w"], c["dst_h"])
    _check_frame(D, c["out"], c["name"])


@pytest.mark.parametrize("bd,sw,sh,dw,dh", [(10, 200, 120, 150, 90), (8, 136, 72, 68, 36), (10, 71, 39, 31, 19),
                                            (8, 64, 48, 64, 24), (10, 1040, 16, 585, 16), (8, 40, 24, 80, 48),
                                            (10, 160, 96, 40, 24)])
def test_frame_matches_restatement(ctx, bd, sw, sh, dw, dh):
    """Every plane of a few more shapes (code 17, denominator 16, odd sizes, one direction only, a second tile, an
    upscale, two halving steps) against the restatement."""
    r = np.random.default_rng(sw * 7 + dh)
    planes = [r.integers(0, 1 << bd, ((sh + (p > 0)) >> (p > 0), (sw + (p > 0)) >> (p > 0))).astype(
        np.uint16 if bd > 8 else np.uint8) for p in range(3)]
    S, D, _ = _frames(ctx, planes, sw, sh, dw, dh, bd, 3)
    svtgpu.resize(S, D, sw, sh, dw, dh)
    _check_frame(D, rc.resize_frame(planes, sw, sh, dw, dh, bd), "%dx%d->%dx%d" % (sw, sh, dw, dh))


def test_equal_sizes_copy(ctx):
    r = np.random.default_rng(5)
    planes = [r.integers(0, 1024, ((17 + (p > 0)) >> (p > 0), (83 + (p > 0)) >> (p > 0))).astype(np.uint16)
              for p in range(3)]
    S, D, _ = _frames(ctx, planes, 83, 17, 83, 17, 10, 4)
    svtgpu.resize(S, D, 83, 17, 83, 17)
    _check_frame(D, planes, "copy")
    got, untouched = _plane(ctx, planes[0], 83, 17, 10, 3, 5, 1)
    assert np.array_equal(got, planes[0]) and untouched


def test_invalid_arguments_are_refused_without_a_launch(ctx):
    L = svtgpu.lib()
    mk = lambda w, h, bd: svtgpu.Frame(ctx, w, h, bd)
    S, D, D8 = mk(88, 16, 10), mk(64, 16, 10), mk(64, 16, 8)
    fill = [np.full((16 >> (p > 0), 64 >> (p > 0)), 0x155, np.uint16) for p in range(3)]
    D.upload(fill)
    bad = [(S, S, 88, 16, 64, 12), (S, D8, 88, 16, 64, 12), (S, D, 89, 16, 64, 12), (S, D, 88, 17, 64, 12),
           (S, D, 88, 16, 65, 12), (S, D, 88, 16, 64, 17), (S, D, 0, 16, 64, 12), (S, D, 88, 16, 64, 0),
           (S, D, 20, 16, 64, 12), (S, D, 88, 4, 64, 12)]  # the last two: up-scales beyond 2x
    for src, dst, sw, sh, dw, dh in bad:
        assert L.svtgpu_resize_frame(src.h, dst.h, sw, sh, dw, dh, None) == -1, (sw, sh, dw, dh)
        with pytest.raises(svtgpu.SvtGpuError):
            svtgpu.resize(src, dst, sw, sh, dw, dh)
    assert L.svtgpu_resize_frame(None, D.h, 88, 16, 64, 12, None) == -1
    assert L.svtgpu_resize_frame(S.h, None, 88, 16, 64, 12, None) == -1
    ctx.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(D.download(), fill))  # nothing ran
    t = _dev(np.zeros(8192, np.uint16))
    p, q = t.data_ptr(), t.data_ptr() + 8192
    ok = dict(src=p, bits=16, ss=96, in_w=88, in_h=16, dst=q, ds=80, out_w=66, out_h=12, bd=10)
    for k, v in [("src", None), ("dst", None), ("dst", p), ("dst", p + 2 * (15 * 96 + 87)), ("bits", 12), ("bits", 0),
                 ("ss", 87), ("ds", 65), ("in_w", 0), ("in_h", 0), ("out_w", 0), ("out_h", -1), ("in_w", 32),
                 ("in_h", 5), ("in_w", 65537), ("bd", 13), ("bd", 7)]:
        a = dict(ok, **{k: v})
        if k == "in_w" and v > 96:
            a["ss"] = v
        rc_ = L.svtgpu_resize_plane(a["src"], a["bits"], a["ss"], a["in_w"], a["in_h"], a["dst"], a["ds"], a["out_w"],
                                    a["out_h"], a["bd"], ctx.stream)
        assert rc_ == -1, (k, v)
    t8 = _dev(np.zeros(4096, np.uint8))
    assert L.svtgpu_resize_plane(t8.data_ptr(), 8, 96, 88, 16, t8.data_ptr() + 2048, 80, 66, 12, 10, ctx.stream) == -1
    ctx.synchronize()
    assert not _host(t, np.uint16).any() and not _host(t8, np.uint8).any()


@pytest.mark.parametrize("i", range(len(PLANES)))
def test_host_shims_match_records(i):
    """svtgpu_av1_resize_plane / svtgpu_av1_highbd_resize_plane: the reference's prototypes, host pointers."""
    c = PLANES[i]
    L = svtgpu.lib()
    ss, ds = c["in_w"] + 5, c["out_w"] + 3
    src = np.zeros((c["in_h"], ss), c["src"].dtype)
    src[:, :c["in_w"]] = c["src"]
    dst = np.full((c["out_h"], ds), SENTINEL, c["src"].dtype)
    if c["bd"] > 8:
        r = L.svtgpu_av1_highbd_resize_plane(svtgpu.ptr(src), c["in_h"], c["in_w"], ss, svtgpu.ptr(dst), c["out_h"],
                                             c["out_w"], ds, c["bd"])
    else:
        r = L.svtgpu_av1_resize_plane(svtgpu.ptr(src), c["in_h"], c["in_w"], ss, svtgpu.ptr(dst), c["out_h"],
                                      c["out_w"], ds)
    assert r == 0
    np.testing.assert_array_equal(dst[:, :c["out_w"]], c["out"], err_msg=c["name"])
    assert (dst[:, c["out_w"]:] == SENTINEL).all()


def test_host_shims_refuse_bad_sizes():
    L = svtgpu.lib()
    a, b = np.zeros((8, 8), np.uint8), np.full((8, 8), SENTINEL, np.uint8)
    assert L.svtgpu_av1_resize_plane(svtgpu.ptr(a), 8, 8, 8, svtgpu.ptr(b), 0, 4, 8) == 0x80001005
    assert L.svtgpu_av1_resize_plane(svtgpu.ptr(a), 8, 8, 4, svtgpu.ptr(b), 4, 4, 8) == 0x80001005
    assert L.svtgpu_av1_resize_plane(None, 8, 8, 8, svtgpu.ptr(b), 4, 4, 8) == 0x80001005
    assert (b == SENTINEL).all()


def test_back_to_back_calls_share_the_workspace_in_stream_order(ctx):
    """Two different plane calls on one stream, one synchronise at the end: the second reuses the first's intermediate
    plane and halving buffers only after the first has read them."""
    by = {(c["bd"], c["in_w"], c["in_h"], c["out_w"], c["out_h"], c["content"]): c for c in PLANES}
    a, b = by[(10, 100, 40, 23, 9, 0)], by[(10, 88, 16, 66, 12, 0)]
    st = ctx.stream_create()
    try:
        warm = _enqueue(ctx, a["src"], a["out_w"], a["out_h"], 10, 112, 48, 0, st)  # the workspace grows here
        ctx.synchronize(st)
        jobs = [_enqueue(ctx, c["src"], c["out_w"], c["out_h"], 10, (c["in_w"] + 15) & ~15, 80, 0, st)
                for c in (a, b, a)]
        ctx.synchronize(st)
        for job, c in zip(jobs, (a, b, a)):
            got, untouched = _collect(job)
            np.testing.assert_array_equal(got, c["out"], err_msg=c["name"])
            assert untouched
    finally:
        svtgpu.Context.stream_destroy(st)
