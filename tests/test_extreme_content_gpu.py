"""The search kernels on worst-case and all-tie content (extreme_cases.py), against the CPU oracle, bit for bit.

The other GPU tests of these families run on smooth synthetic frames, where no difference nears its largest
magnitude, no accumulator nears the bound its comment states and hardly two search positions tie.  Here: all-zero,
all-max, 0 / max checkerboards, flat, periodic and sparse contents put the Wiener statistics' hi / lo split and i32
wave fold, the Wiener trial's int16 pairs, the LR solve on H = 0, the MD cell moments' packed int16 sum and 32-bit
SSE, the ME search's first-minimum merge, the CCSO bins' shared LDS word and the DLF level search's SSE sums and ties
at their limits.  test_extreme_content.py holds the oracle to a numpy restatement on the same cases.

One-line kernel changes these cases catch and smooth content does not (reasoned from the code, not run):
  1. wiener_stats_kernel: the four wave partials summed without the (long long) cast -- 4 x 943 718 400 wraps an int
     on the tile_max unit; smooth content stays orders of magnitude below.
  2. LR search: a Wiener solve that does not take linsolve's zero-pivot exit -- only a flat unit has H = 0; and a
     finish that resolves equal costs with "<=" where the reference has "<" -- only flat / flat makes them equal.
  3. md_expand_kernel: the block SSE summed as a signed 32-bit int -- 4 286 582 784 is above 2^31 only when nearly
     every sample differs by the full range.
  4. block_stats (the shims): a 32-bit SSE total -- 128x128 at 10 bit is 17 146 331 136.
  5. me_search_kernel: merge() without its index comparison (the lower wave keeps a tie) -- the edge_tie case has first
     minima at row 1 (wave 1) tied with row 4 (wave 0); noise never ties.
  6. ccso_bins_kernel: NQ_SHIFT lowered to 32 -- 4352 samples x 1023^2 in one bin (136x72, 10 bit, max against zero)
     carry into the count; errors of a few levels never do.
  7. DLF level search: a trial level accepted on an equal cost -- only flat content makes every level cost the same.
  8. CDEF pick: an argmin that keeps a later minimum, or an RD choice with "<=" -- a flat, black, white or checkerboard recon gives
     every searched strength of every filter block the same MSE, so every call of the pick ties and the frame must
     come back with the single strength 0 and unfiltered (test_cdef_pick_ties_gpu.py has the table cases)."""
import ctypes

import numpy as np
import pytest

import extreme_cases as ec
import md_cases as mc
import oracle
import svtgpu

pytestmark = pytest.mark.gpu
P = lambda a: ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def ctx():
    return svtgpu.Context(0)


def _frame(ctx, planes, bd):
    h, w = planes[0].shape
    f = svtgpu.Frame(ctx, w, h, bd)
    f.upload([np.ascontiguousarray(p) for p in planes])
    return f


def _luma_frame(ctx, y, bd):
    h, w = y.shape
    c = np.zeros((h // 2, w // 2), y.dtype)
    return _frame(ctx, [y, c, c], bd)


# --------------------------------------------------------------------------------------------- 1. Wiener statistics
@pytest.mark.parametrize("w,h,bd,dname,sname", ec.STATS_CASES)
def test_wiener_stats_shim_vs_oracle(ctx, w, h, bd, dname, sname):
    """svtgpu_av1_compute_stats(_highbd) of one unit (wiener_stats_kernel) for windows 7, 5 and 3: v = 32 hi + lo with
    hi at -32 and at 31, X at +-(maxv - 1) on every pixel, a whole tile at v = +-960 (the largest i32 wave fold)."""
    dgd, src, want = ec.stats_case(w, h, bd, dname, sname)
    L, hbd = svtgpu.lib(), bd > 8
    d = np.ascontiguousarray(dgd if hbd else dgd.astype(np.uint8))
    s = np.ascontiguousarray(src if hbd else src.astype(np.uint8))
    st = d.shape[1]
    at = lambda a: ctypes.c_void_p((a.ctypes.data + (4 * st + 4) * a.itemsize) >> (1 if hbd else 0))
    for win in ec.WINS:
        M, H = np.zeros(win * win, np.int64), np.zeros(win ** 4, np.int64)
        args = (win, at(d), at(s), 0, w, 0, h, st, st, P(M), P(H))
        if hbd:
            L.svtgpu_av1_compute_stats_highbd(*args, bd)
        else:
            L.svtgpu_av1_compute_stats(*args)
        np.testing.assert_array_equal(M, want[win][0], err_msg="M win %d" % win)
        np.testing.assert_array_equal(H, want[win][1], err_msg="H win %d" % win)


# --------------------------------------------------------------------------------------------- 2. LR search
@pytest.mark.parametrize("w,h,bd,rname,sname", ec.LR_CASES)
def test_lr_search_vs_oracle(ctx, w, h, bd, rname, sname):
    """What test_lr_search_vs_oracle compares (frame types, sse and sgrproj records, the Wiener records where
    evaluated, the frame restored with the searched units), on flat (H = 0: the solve's failure path, all-equal costs
    in the finish), checkerboard (the Wiener trial's int16 pairs at the 10-bit clamp limit) and sparse content."""
    rec, src, want_ft, want_units, want_recs, want_out = ec.lr_case(w, h, bd, rname, sname)
    R, S = _frame(ctx, rec, bd), _frame(ctx, src, bd)
    st = svtgpu.LrState(ctx, w, h, ec.LR_UNIT_SIZE)
    ft, recs = st.search(R, S, ec.lr_ctrls(svtgpu), records=True)
    assert ft == want_ft
    for p in range(3):
        np.testing.assert_array_equal(recs[p]["sse"], want_recs[p]["sse"], err_msg="plane %d sse" % p)
        np.testing.assert_array_equal(recs[p]["sgrproj"], want_recs[p]["sgrproj"], err_msg="plane %d sgrproj" % p)
        ok = recs[p]["sse"][:, 1] != ec.I64_MAX
        np.testing.assert_array_equal(recs[p]["wiener"][ok], want_recs[p]["wiener"][ok], err_msg="plane %d" % p)
        if (rname, sname) in ec.LR_NEED_WIENER:
            assert ok.any(), p
    D, O = _frame(ctx, rec, bd), svtgpu.Frame(ctx, w, h, bd)
    st.apply(D, R, O, ft)
    got = O.download()
    for p in range(3):
        np.testing.assert_array_equal(got[p], want_out[p], err_msg="plane %d" % p)
    st.close()


# --------------------------------------------------------------------------------------------- 3. MD batch
@pytest.mark.parametrize("w,bd,sname,rname", ec.MD_CASES)
def test_md_batch_vs_oracle(ctx, w, bd, sname, rname):
    """md_dist_kernel + md_expand_kernel: cell sums of +-16 368 in the packed int16 field, the 64x64 SSE at
    4096 * 1023^2 (8 384 512 below 2^32, before the rounding's + 8), the largest SAD with sum 0, MVs reaching past
    every frame edge and placing the whole block outside the frame."""
    src, refs, runs = ec.md_case(w, bd, sname, rname)
    S = _luma_frame(ctx, src, bd)
    R = [_luma_frame(ctx, r, bd) for r in refs]
    b = svtgpu.MdBatch(ctx, w, w, ec.MD_NREF)
    for mv, want in runs:
        b.set_mvs(mv)
        b.run(S, R)
        np.testing.assert_array_equal(b.read(), want)
    b.close()


# --------------------------------------------------------------------------------------------- 4. MD / ME shims
@pytest.mark.parametrize("bd", [8, 10])
def test_md_shims_full_magnitude(ctx, bd):
    """Every MD_SIZES shape with one block at the maximum and the other at zero, both ways."""
    L, maxv = svtgpu.lib(), (1 << bd) - 1
    for w, h in mc.MD_SIZES:
        for a, b in ((maxv, 0), (0, maxv)):
            dt = np.uint16 if bd > 8 else np.uint8
            s, r = np.full((h, w), a, dt), np.full((h, w), b, dt)
            sad, osse, var = oracle.block_dist(s, r, w, h, bd)
            raw = oracle.block_sse(s, r, w, h, bd)
            sse, msg = ctypes.c_uint32(), (w, h, a, b)
            if bd == 8:
                assert getattr(L, "svtgpu_aom_sad%dx%d" % (w, h))(P(s), w, P(r), w) == sad, msg
                assert getattr(L, "svtgpu_aom_variance%dx%d" % (w, h))(P(s), w, P(r), w, ctypes.byref(sse)) == var, msg
                assert sse.value == osse, msg
                refs = (ctypes.c_void_p * 4)(*[r.ctypes.data] * 4)
                out4 = np.zeros(4, np.uint32)
                getattr(L, "svtgpu_aom_sad%dx%dx4d" % (w, h))(P(s), w, refs, w, P(out4))
                assert list(out4) == [sad] * 4, msg
                assert L.svtgpu_aom_sse(P(s), w, P(r), w, w, h) == raw, msg
                assert L.svtgpu_spatial_full_distortion_kernel(P(s), 0, w, P(r), 0, w, w, h) == raw, msg
            else:
                a8, b8 = ctypes.c_void_p(s.ctypes.data >> 1), ctypes.c_void_p(r.ctypes.data >> 1)
                assert getattr(L, "svtgpu_aom_highbd_10_variance%dx%d" % (w, h))(a8, w, b8, w, ctypes.byref(sse)) \
                    == var, msg
                assert sse.value == osse, msg
                assert L.svtgpu_sad_16b_kernel(P(s), w, P(r), w, h, w) == sad, msg
                assert L.svtgpu_aom_highbd_sse(P(s), w, P(r), w, w, h) == raw, msg
                assert L.svtgpu_full_distortion_kernel16_bits(P(s), 0, w, P(r), 0, w, w, h) == raw, msg


# --------------------------------------------------------------------------------------------- 5. ME search
@pytest.mark.parametrize("w,h,kind", [(w, h, k) for (w, h) in ec.ME_SIZES for k in ec.ME_KINDS])
def test_me_search_ties_vs_oracle(ctx, w, h, kind):
    """me_search_kernel's first minimum in scan order (four waves by row mod 4, x groups of 4, bands of 32 rows, merged
    lexicographically) where every position ties (flat, max against zero, a search area wholly in the clamped
    padding) or ties periodically (stripes), for both search areas, whole and sub-sampled SADs."""
    src, refs, org = ec.me_frames(w, h, kind)
    S = _luma_frame(ctx, src, 8)
    R = [_luma_frame(ctx, r, 8) for r in refs]
    me = svtgpu.MeBatch(ctx, w, h, ec.ME_NREF)
    me.set_origins(org)
    for saw, sah in ec.ME_AREAS:
        for sub in (0, 1):
            _, _, _, osad, omv = ec.me_case(w, h, saw, sah, sub, kind)
            me.search(S, R, saw, sah, sub)
            gs, gm = me.read()
            msg = "area %dx%d sub %d" % (saw, sah, sub)
            np.testing.assert_array_equal(gs, osad, err_msg="sad " + msg)
            np.testing.assert_array_equal(gm, omv, err_msg="mv " + msg)
    me.close()


# --------------------------------------------------------------------------------------------- 6. CCSO
def _dev(a):
    import torch
    a = np.array(a, order="C")  # a copy: the cases' arrays are read-only
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()
    return t


def _host(t, dtype):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


@pytest.mark.parametrize("w,h,bd,kind", ec.CCSO_CASES)
def test_ccso_search_and_apply_vs_oracle(ctx, w, h, bd, kind):
    """ccso_bins_kernel's shared LDS word (count << 49 | sum of squares) and biased error sum with every sample of a
    workgroup in one bin and every error at +maxv or at -maxv; the search's result and its apply."""
    import torch
    pre, org, rec, (orc, oprms, oflags, off), outs, ext_h = ec.ccso_case(w, h, bd, kind)
    rdmult, q = ec.ccso_rd()
    st = svtgpu.CcsoState(ctx, w, h)
    d_pre = _dev(pre)
    ext = torch.zeros(((h + 10) * (w + 10),), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    st.extend(d_pre.data_ptr(), 16, w, ext.data_ptr())
    np.testing.assert_array_equal(_host(ext, np.uint16).reshape(h + 10, w + 10), ext_h)
    d_org, d_rec = [_dev(a) for a in org], [_dev(a) for a in rec]
    rc, prms, flags, ff = st.search_frame(ext.data_ptr(), [t.data_ptr() for t in d_org],
                                          [t.data_ptr() for t in d_rec], bd, rdmult, q)
    torch.cuda.synchronize()
    assert (rc, ff) == (orc, off)
    for p in range(3):
        assert prms[p].fields() == oprms[p].fields(), p
        np.testing.assert_array_equal(prms[p].lut(), oprms[p].lut(), err_msg="plane %d" % p)
        np.testing.assert_array_equal(flags[p], oflags[p], err_msg="plane %d" % p)
        plane, want = outs[p]
        d = _dev(plane)
        st.apply(ext.data_ptr(), p, bd, d.data_ptr(), 16 if bd > 8 else 8, plane.shape[1])
        np.testing.assert_array_equal(_host(d, plane.dtype.type), want, err_msg="plane %d" % p)
    st.close()


# --------------------------------------------------------------------------------------------- 7. DLF
@pytest.mark.parametrize("w,h,bd,rname,sname", ec.DLF_CASES)
def test_dlf_pick_and_filter_vs_oracle(ctx, w, h, bd, rname, sname):
    """svtgpu_dlf_pick where every level costs the same (flat: nothing is filtered) and where the filters and the SSE
    sums saturate (checkerboard, max against zero), then the frame filtered at the picked levels."""
    rec, src, mi, want, want_out = ec.dlf_case(w, h, bd, rname, sname)
    R, S, O = _frame(ctx, rec, bd), _frame(ctx, src, bd), svtgpu.Frame(ctx, w, h, bd)
    st = svtgpu.DlfState(ctx, w, h)
    st.set_mode_info(mi)
    got = st.pick(R, S, ec.dlf_params(), *ec.DLF_PICK_ARGS)
    assert got.levels() == want.levels()
    back = R.download()
    for p in range(3):  # the search leaves the recon unfiltered
        np.testing.assert_array_equal(back[p], rec[p])
    st.filter_to(R, O, got)
    out = O.download()
    for p in range(3):
        np.testing.assert_array_equal(out[p], want_out[p], err_msg="plane %d" % p)
    st.close()


# --------------------------------------------------------------------------------------------- 8. CDEF pick
@pytest.mark.parametrize("w,h,bd,level,rname,sname", ec.CDEF_CASES)
def test_cdef_search_pick_apply_vs_oracle(ctx, w, h, bd, level, rname, sname):
    """search -> pick -> apply where every strength of a filter block has the same MSE (flat, black and white recon;
    from level 2 on also the unsearched chroma strengths' constant), one and three filter blocks with partial
    right / bottom blocks: the tables, the frame parameters, the per-FB strengths and every output plane."""
    rec, src, (omse, oskip, od, ov), (oprm, ofbs), want_out = ec.cdef_case(w, h, bd, level, rname, sname)
    R, S, O = _frame(ctx, rec, bd), _frame(ctx, src, bd), svtgpu.Frame(ctx, w, h, bd)
    ctrls = svtgpu.cdef_controls(level)
    st = svtgpu.CdefState(ctx, w, h)
    st.search(R, S, ctrls, ec.CDEF_Q)
    mse, skip, d, v = st.read()
    np.testing.assert_array_equal(skip, oskip)
    np.testing.assert_array_equal(mse, omse)
    prm, fbs = st.pick(ctrls, ec.CDEF_Q, ec.CDEF_LAMBDA)
    assert prm.as_tuple() == oprm
    np.testing.assert_array_equal(fbs, ofbs)
    st.apply(R, O, prm)
    out = O.download()
    for p in range(3):
        np.testing.assert_array_equal(out[p], want_out[p], err_msg="plane %d" % p)
    st.close()
