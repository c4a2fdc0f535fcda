"""The per-thread staging buffer that every per-block RTCD shim reserves from (svtgpu_stage_reserve, runtime.hip): shims
of different families interleaved on one thread, so the one buffer grows, is reused by smaller calls with another
family's bytes still in it, and serves the first call again; two threads running shims at once, each on its own stage; a
thread that ends (its stage is freed) and the same shims afterwards.  Every result is held bit-exact to the golden
record the family's own test uses."""
import ctypes
import threading

import numpy as np

import pytest

import ccso_cases as xc
import cdef_cases as cc
import compound_cases as cpc
import dlf_cases as dc
import frame_cases as fc
import interp_cases as ic
import md_cases as mdc
import me_cases as mec
import svtgpu

pytestmark = pytest.mark.gpu
P = lambda a: ctypes.c_void_p(a.ctypes.data)


def _framed(src, w, h):
    """The (h + 8) x (w + 8) source inside a larger buffer whose stride is no multiple of 16."""
    big = np.full((h + 14, w + 21), 1, src.dtype)
    big[2:2 + h + 8, 5:5 + w + 8] = src
    return big


def convolve_4x4():
    c = next(c for c in ic.block_cases() if (c["w"], c["h"], c["form"]) == (4, 4, 3))
    w, h = c["w"], c["h"]
    big = _framed(ic.block_source(c["bd"], w, h, c["content"], c["index"]), w, h)
    dst = np.full((h + 4, w + 7), 9, big.dtype)
    fx, fy = ic.block_filters(c)
    r0, r1 = ic.rounds(c["bd"])
    svtgpu.convolve_sr(ic.FORMS[c["form"]], big, 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, c["bd"], dst, 3, 2)
    np.testing.assert_array_equal(dst[2:2 + h, 3:3 + w], c["out"], err_msg=c["name"])


def compound_128x128():
    """Both calls of a compound block: the first writes conv_dst, the second (do_average) reads it and writes pixels."""
    c = next(c for c in cpc.block_cases() if (c["w"], c["h"]) == (128, 128))
    w, h, bd = c["w"], c["h"], c["bd"]
    fx, fy = cpc.block_filters(c)
    r0, r1 = cpc.rounds(bd)
    form = cpc.FORMS[c["form"]]
    srcs = [_framed(cpc.block_source(bd, w, h, c["content"], c["index"], k), w, h) for k in (0, 1)]
    conv = np.full((h, w + 3), 7, np.uint16)
    dst = np.full((h + 4, w + 7), 9, srcs[0].dtype)
    svtgpu.jnt_convolve(form, srcs[0], 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, bd, conv, 0, dst=dst, dx0=3, dy0=2)
    np.testing.assert_array_equal(conv[:, :w], c["conv"], err_msg=c["name"] + " conv_dst")
    svtgpu.jnt_convolve(form, srcs[1], 5 + 3, 2 + 3, w, h, fx, fy, r0, r1, bd, conv, 1, c["mode"][0], c["mode"][1], c["mode"][2],
                        dst=dst, dx0=3, dy0=2)
    np.testing.assert_array_equal(dst[2:2 + h, 3:3 + w], c["out"], err_msg=c["name"])


def cdef_filter_block():
    g = cc.load("cdef_filter_block.bin")
    np.testing.assert_array_equal(cc.run_filter_block(svtgpu.lib().svtgpu_cdef_filter_block, g, 0), g["out"][0])


def lpf_segment():
    """Record 0 of dlf_lpf.bin, laid out as tests/test_dlf_gpu.py lays it out."""
    g = cc.load("dlf_lpf.bin")
    kind, fn, bl, li, th = (int(x) for x in g["meta"][0])
    vertical, lowbd = fn >= 4, kind == 8
    win = np.zeros((16, 16), np.uint8 if lowbd else np.uint16)
    for i in range(4):
        if vertical:
            win[8 + i, :] = g["in"][0][i]
        else:
            win[:, 8 + i] = g["in"][0][i]
    thr = [np.full(16, v, np.uint8) for v in (bl, li, th)]
    args = [ctypes.c_void_p(win.ctypes.data + (8 * 16 + 8) * win.itemsize), 16] + [P(t) for t in thr]
    name = "svtgpu_%slpf_%s" % ("" if lowbd else "highbd_", dc.LPF_NAMES[fn])
    getattr(svtgpu.lib(), name)(*(args if lowbd else args + [8 if kind == 108 else kind]))
    got = np.stack([win[8 + i, :] if vertical else win[:, 8 + i] for i in range(4)]).astype(np.uint16)
    np.testing.assert_array_equal(got, g["out"][0])


def md_sad_and_variance_4x4():
    L, g = svtgpu.lib(), mdc.golden()
    assert mdc.MD_SIZES[0] == (4, 4)
    res = g["s0_res"]
    s16, r16, s8, r8 = mdc.case(g, 0, 0)
    st, sse = s16.shape[1], ctypes.c_uint32()
    assert L.svtgpu_aom_sad4x4(P(s8), st, P(r8), st) == res[0][0]
    assert L.svtgpu_aom_variance4x4(P(s8), st, P(r8), st, ctypes.byref(sse)) == res[0][1]
    assert sse.value == res[0][2]


def ccso_block():
    """The classifier shim and the distortion shim of block record 0."""
    L = svtgpu.lib()
    c = xc.block_cases(xc.golden())[0]
    ext, es, cs = c["ext"], c["es"], c["cs"]
    src = ctypes.c_void_p(ext.ctypes.data + 2 * (5 * es + 5))
    loc = np.array(xc.sample_pos(es, c["sup"]), np.int32)
    c0, c1 = np.zeros_like(c["cls0"]), np.zeros_like(c["cls1"])
    L.svtgpu_ccso_derive_src_block(src, P(c0), P(c1), es, cs, c["x"], c["y"], c["pw"], c["ph"], c["hs"], c["vs"],
                                   c["qs"], -c["qs"], P(loc), c["blk"], c["clf"])
    np.testing.assert_array_equal(c0, c["cls0"])
    np.testing.assert_array_equal(c1, c["cls1"])
    d = np.ascontiguousarray(c["with_buf"])
    ssd = L.svtgpu_compute_distortion_block(P(c["dst0"]), cs, P(d), cs, c["x"], c["y"], 7 if c["hs"] else 8, c["ph"], c["pw"])
    assert ssd == c["ssd"]


def me_sad_loop():
    s, r, meta = mec.loop_cases(mec.golden())[0]
    bw, bh, saw, sah, ss, rs, srr, skip, best, c = meta
    b, x, y = ctypes.c_uint64(0), ctypes.c_int16(-1), ctypes.c_int16(-1)
    svtgpu.lib().svtgpu_sad_loop_kernel(P(s), ss, P(r), rs, bh, bw, ctypes.byref(b), ctypes.byref(x), ctypes.byref(y), srr, skip,
                                        saw, sah)
    assert b.value == best, meta
    if best < 0xffffff:
        assert (x.value & 0xFFFF) | ((y.value & 0xFFFF) << 16) == c & 0xFFFFFFFF, meta


def frame_convert():
    src, d0, d1, w, h, ss, ds = fc.conv_cases(fc.golden())[0]
    d = d0.copy()
    if src.dtype == np.uint8:
        svtgpu.lib().svtgpu_convert_8bit_to_16bit(P(src), ss, P(d), ds, w, h)
    else:
        svtgpu.lib().svtgpu_convert_16bit_to_8bit(P(src), ss, P(d), ds, w, h)
    np.testing.assert_array_equal(d, d1)


FIRST_HALF = [convolve_4x4, compound_128x128, cdef_filter_block, lpf_segment]
SECOND_HALF = [md_sad_and_variance_4x4, ccso_block, me_sad_loop, frame_convert]
# shim entry points the sequence below passes through: 1 + 2 + 1 + 1 + 2 + 2 + 1 + 1 + 1 (counted in a run of the commit
# before the shared stage; the stage must not change it)
SEQUENCE_SHIM_CALLS = 12


def _in_thread(steps, times=1):
    """A thread that runs `steps` `times` times; returns (thread, the list its failure lands in)."""
    failed = []

    def body():
        try:
            for _ in range(times):
                for f in steps:
                    f()
        except BaseException as e:  # noqa: BLE001 -- reported by the test's thread
            failed.append(e)
    return threading.Thread(target=body), failed


def test_interleaved_families_on_one_thread():
    """The 128x128 compound call grows the stage past everything else; the small and fixed-size calls after it reuse that
    buffer with the compound call's bytes in it; the first call then runs again."""
    L = svtgpu.lib()
    before = L.svtgpu_shim_calls()
    for f in FIRST_HALF + SECOND_HALF + [convolve_4x4]:
        f()
    assert L.svtgpu_shim_calls() - before == SEQUENCE_SHIM_CALLS


def test_two_threads_at_once():
    a, fa = _in_thread(FIRST_HALF, 4)
    b, fb = _in_thread(SECOND_HALF, 4)
    a.start(), b.start()
    a.join(), b.join()
    assert not fa and not fb, (fa, fb)


def test_a_thread_that_ends():
    steps = [compound_128x128, md_sad_and_variance_4x4]
    t, failed = _in_thread(steps)
    t.start()
    t.join()
    assert not failed, failed
    for f in steps:
        f()
