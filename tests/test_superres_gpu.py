"""Super-resolution on the MI355X: svtgpu_superres_upscale_plane / _frame against every upscale record of the
reference's fixture (tests/golden/superres.bin), and the reference's loop restoration of super-resolved frames with
both downscaled frames upscaled on the device.  Bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import superres_cases as sc
import svtgpu

pytestmark = pytest.mark.gpu

UP = list(sc.up_cases())
LR = list(sc.lr_cases())
SENTINEL = 0xA5


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


def _plane(ctx, c, src_stride, shift=0, dst_pad=24):
    """svtgpu_superres_upscale_plane of record c's source with a source stride of src_stride samples, the plane starting
    `shift` samples into the buffer.  Returns (columns [0, dst_w), the untouched columns past them, dst_w)."""
    dt, rows, coded = c["src"].dtype, c["rows"], c["coded"]
    dst_w = ((c["upscaled_width"] + 7) & ~7) >> c["sub_x"]
    r = np.random.default_rng(c["coded"] * 131 + c["out_w"])
    src = r.integers(0, 1 << c["bd"], (rows * src_stride + shift,)).astype(dt)  # what lies between the rows is random
    for y in range(rows):
        src[shift + y * src_stride:shift + y * src_stride + coded] = c["src"][y]
    dst = np.full((rows, dst_w + dst_pad), SENTINEL, dt)
    s, d = _dev(src), _dev(dst)
    rc = svtgpu.lib().svtgpu_superres_upscale_plane(s.data_ptr() + shift * dt.itemsize, dt.itemsize * 8, src_stride,
                                                    coded, c["in_w"], d.data_ptr(), dst_w + dst_pad, dst_w, c["out_w"],
                                                    rows, c["bd"], ctx.stream)
    assert rc == 0, rc
    ctx.synchronize()
    got = _host(d, dt)
    return got[:, :dst_w], got[:, dst_w:], dst_w


@pytest.mark.parametrize("i", range(len(UP)))
def test_upscale_plane_matches_records(ctx, i):
    c = UP[i]
    got, rest, dst_w = _plane(ctx, c, (c["coded"] + 15) & ~15)
    np.testing.assert_array_equal(got[:, :c["out_w"]], c["out"], err_msg=c["name"])
    # the columns past out_w, up to the 8-aligned frame's plane width, repeat the row's last upscaled sample
    assert (got[:, c["out_w"]:] == c["out"][:, -1:]).all(), c["name"]
    assert (rest == SENTINEL).all(), c["name"]  # and nothing past the plane width is written


@pytest.mark.parametrize("i", [i for i, c in enumerate(UP) if c["denom"] in (9, 11, 12, 16) and c["rows"] <= 8])
@pytest.mark.parametrize("extra,shift", [(16, 0), (3, 0), (21, 5)])
def test_source_stride_and_alignment_do_not_matter(ctx, i, extra, shift):
    """A source stride wider than the plane, rows that start at no 16-byte boundary (the one-sample loads) and a plane
    that starts inside its buffer give the recorded output."""
    c = UP[i]
    got, _, _ = _plane(ctx, c, ((c["coded"] + 15) & ~15) + extra, shift)
    np.testing.assert_array_equal(got[:, :c["out_w"]], c["out"], err_msg=c["name"])


def _frames_for(ctx, c):
    """A downscaled 4:2:0 picture holding record c's plane (luma, or both chroma planes; the other planes and the rows
    past the record's are random) and the expected upscaled planes."""
    bd, sx, fw, uw = c["bd"], c["sub_x"], c["frame_width"], c["upscaled_width"]
    w8, u8 = (fw + 7) & ~7, (uw + 7) & ~7
    h8 = ((c["rows"] << sx) + 7) & ~7
    r = np.random.default_rng(fw * 7 + uw)
    planes = [r.integers(0, 1 << bd, (h8 >> (p > 0), w8 >> (p > 0))).astype(c["src"].dtype) for p in range(3)]
    for p in ([0] if sx == 0 else [1, 2]):
        planes[p][:c["rows"]] = c["src"]
    want = sc.upscale_frame(planes, fw, uw, bd, [u8, u8 >> 1, u8 >> 1])
    S, D = svtgpu.Frame(ctx, w8, h8, bd), svtgpu.Frame(ctx, u8, h8, bd)
    S.upload(planes)
    return S, D, planes, want


@pytest.mark.parametrize("i", range(len(UP)))
def test_upscale_frame_matches_records(ctx, i):
    c = UP[i]
    S, D, planes, want = _frames_for(ctx, c)
    svtgpu.superres_upscale(S, D, c["frame_width"], c["upscaled_width"])
    got = D.download()
    for p in ([0] if c["sub_x"] == 0 else [1, 2]):  # the reference's own output
        np.testing.assert_array_equal(got[p][:c["rows"], :c["out_w"]], c["out"], err_msg=c["name"])
    for p in range(3):  # every sample of the destination, against the restatement the CPU tests hold to the records
        np.testing.assert_array_equal(got[p], want[p], err_msg="%s plane %d" % (c["name"], p))


def test_equal_widths_copy(ctx):
    r = np.random.default_rng(5)
    planes = [r.integers(0, 1024, (16 >> (p > 0), 88 >> (p > 0))).astype(np.uint16) for p in range(3)]
    S, D = svtgpu.Frame(ctx, 88, 16, 10), svtgpu.Frame(ctx, 88, 16, 10)
    S.upload(planes)
    svtgpu.superres_upscale(S, D, 83, 83)
    assert all(np.array_equal(a, b) for a, b in zip(D.download(), planes))


def test_invalid_arguments_are_refused_without_a_launch(ctx):
    L = svtgpu.lib()
    mk = lambda w, h, bd: svtgpu.Frame(ctx, w, h, bd)
    S, D, D8, Dh, Dw = mk(56, 16, 10), mk(88, 16, 10), mk(88, 16, 8), mk(88, 24, 10), mk(120, 16, 10)
    fill = [np.full((16 >> (p > 0), 88 >> (p > 0)), 0x155, np.uint16) for p in range(3)]
    D.upload(fill)
    bad = [(S, S, 54, 54), (S, D8, 54, 88), (S, Dh, 54, 88), (S, D, 57, 88), (S, D, 54, 89), (D, S, 60, 54),
           (S, Dw, 54, 109), (S, D, 0, 88)]
    for src, dst, fw, uw in bad:
        assert L.svtgpu_superres_upscale_frame(src.h, dst.h, fw, uw, None) == -1, (fw, uw)
        with pytest.raises(svtgpu.SvtGpuError):
            svtgpu.superres_upscale(src, dst, fw, uw)
    assert L.svtgpu_superres_upscale_frame(None, D.h, 54, 88, None) == -1
    ctx.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(D.download(), fill))  # nothing ran
    # the plane entry: null or equal pointers, bits, widths beyond the strides, in_w > out_w, out_w > 2 * in_w
    t = _dev(np.zeros(4096, np.uint16))
    p, q = t.data_ptr(), t.data_ptr() + 4096
    ok = dict(src=p, bits=16, ss=64, sw=56, in_w=54, dst=q, ds=96, dw=88, out_w=88, rows=4, bd=10)
    for k, v in [("src", None), ("dst", None), ("dst", p), ("bits", 12), ("sw", 65), ("sw", 53), ("dw", 97),
                 ("dw", 87), ("in_w", 89), ("in_w", 43), ("rows", 0), ("bd", 13), ("bd", 7)]:
        a = dict(ok, **{k: v})
        rc = L.svtgpu_superres_upscale_plane(a["src"], a["bits"], a["ss"], a["sw"], a["in_w"], a["dst"], a["ds"],
                                             a["dw"], a["out_w"], a["rows"], a["bd"], ctx.stream)
        assert rc == -1, (k, v)
    ctx.synchronize()
    assert not _host(t, np.uint16).any()


def _coded_rows(planes, h8, seed):
    """The fixture's planes (crop rows) in a frame of h8 rows: the rows past the crop are random."""
    r = np.random.default_rng(seed)
    out = []
    for p, a in enumerate(planes):
        b = r.integers(0, int(a.max()) + 1, (h8 >> (p > 0), a.shape[1])).astype(a.dtype)
        b[:a.shape[0]] = a
        out.append(b)
    return out


@pytest.mark.parametrize("i", range(len(LR)))
def test_lr_of_superres_frame_matches_reference(ctx, i):
    """The reference saved the deblocked boundary lines upscaled row pair by row pair, upscaled the CDEF frame and ran
    svt_av1_loop_restoration_filter_frame; here both downscaled frames are upscaled whole on the device and the LR state
    is created at the upscaled size, with no superres-specific LR code."""
    c = LR[i]
    fw, uw, h, bd = c["frame_width"], c["w"], c["h"], c["bd"]
    w8, u8, h8 = (fw + 7) & ~7, (uw + 7) & ~7, (h + 7) & ~7
    assert fw != uw and c["dlf"][0].shape == ((h, w8))
    d, s = (svtgpu.Frame(ctx, w8, h8, bd) for _ in range(2))
    D, C, O = (svtgpu.Frame(ctx, u8, h8, bd) for _ in range(3))
    d.upload(_coded_rows(c["dlf"], h8, 1))
    s.upload(_coded_rows(c["cdef"], h8, 2))
    svtgpu.superres_upscale(d, D, fw, uw)
    svtgpu.superres_upscale(s, C, fw, uw)
    st = svtgpu.LrState(ctx, uw, h, c["unit_size"])
    for p in range(3):
        st.set_units(p, c["units"][p])
    st.apply(D, C, O, c["frame_type"])
    got = O.download()
    for p in range(3):
        ph, pw = c["out"][p].shape
        np.testing.assert_array_equal(got[p][:ph, :pw], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
