"""CPU half of the worst-case / all-tie cases (extreme_cases.py): the oracle evaluates every case, equals a plain
numpy / int64 restatement where that is cheap, and every case reaches the magnitude or the tie it is built for.  The
device is held to the same oracle results in test_extreme_content_gpu.py."""
import numpy as np
import pytest

import extreme_cases as ec
import md_cases as mc
import oracle
import svtgpu


# --------------------------------------------------------------------------------------------- contents
@pytest.mark.parametrize("bd", [8, 10])
def test_contents(bd):
    maxv, w, h = (1 << bd) - 1, 72, 40
    p = {n: ec.plane(n, w, h, bd).astype(np.int64) for n in ec.CONTENTS}
    assert not p["zero"].any() and (p["max"] == maxv).all() and (p["flat"] == 100 << (bd - 8)).all()
    assert (p["checker"] + p["anti"] == maxv).all() and p["checker"][0, 1] == maxv and p["checker"][0, 0] == 0
    assert (np.abs(np.diff(p["checker"], axis=0)) == maxv).all() and (np.abs(np.diff(p["checker"], axis=1)) == maxv).all()
    for n, a in ((4, p["stripe4"]), (8, p["stripe8"])):
        assert (a[:, n:] == a[:, :-n]).all() and (a[n:] == a[:-n]).all()           # period n in x and in y
        assert not (a[:, n // 2:] == a[:, :-(n // 2)]).all() and a.max() == maxv and a.min() == 0
    assert (p["sparse_max"] == maxv).sum() == 4 and (p["sparse_max"] == 0).sum() == w * h - 4
    ys, xs = np.nonzero(p["sparse_max"])
    assert all(abs(ys[i] - ys[j]) > 1 or abs(xs[i] - xs[j]) > 1 for i in range(4) for j in range(i))  # isolated
    assert (p["sparse_max"] + p["sparse_zero"] == maxv).all()
    t = ec.plane("tile_max", 256, 256, bd).astype(np.int64)
    assert (t[64:128, 128:192] == maxv).all() and t.sum() == 4096 * maxv
    assert (t + ec.plane("tile_zero", 256, 256, bd) == maxv).all()


# --------------------------------------------------------------------------------------------- 1. Wiener statistics
@pytest.mark.parametrize("w,h,bd,dname,sname", ec.STATS_CASES)
def test_wiener_stats_oracle_vs_numpy(w, h, bd, dname, sname):
    dgd, src, want = ec.stats_case(w, h, bd, dname, sname)
    for win in ec.WINS:
        M, H = ec.stats_numpy(win, dgd, src, w, h, bd)
        np.testing.assert_array_equal(want[win][0], M, err_msg="M win %d" % win)
        np.testing.assert_array_equal(want[win][1], H, err_msg="H win %d" % win)
    if (dname, sname) == ("flat", "flat"):
        assert not want[7][0].any() and not want[7][1].any()  # M = H = 0


def test_wiener_stats_reach():
    """hi = v >> 5 takes both ends of its int8 range, -32 and 31, across the set; the averages are the ones the cases
    are built around; a whole tile at v = +-960 puts the largest per-wave i32 fold a unit can reach between 2^29 and
    2^31 (1024 px * 960^2 = 943 718 400)."""
    lo, hi = 0, 0
    for w, h, bd, dname, sname in ec.STATS_CASES:
        dgd, src, _ = ec.stats_case(w, h, bd, dname, sname)
        a, b = ec.stats_hi_range(dgd, src, w, h)
        lo, hi = min(lo, a), max(hi, b)
        avg = int(dgd[4:4 + h, 4:4 + w].astype(np.int64).sum() // (w * h))
        maxv = (1 << bd) - 1
        X = src[4:4 + h, 4:4 + w].astype(np.int64) - avg
        if dname == "sparse_max":
            assert avg == 0 and (X == maxv).all()
        if dname == "sparse_zero":
            assert avg == maxv - 1 and (X == -(maxv - 1)).all()
        if dname == "tile_max":
            assert avg == 63 and (X == 960).all()
    assert (lo, hi) == (-32, 31)
    for dname, sname in (("tile_max", "max"), ("tile_zero", "zero")):
        dgd, src, _ = ec.stats_case(256, 256, 10, dname, sname)
        fold = ec.stats_largest_wave_fold(7, dgd, src, 256, 256)
        print("%s: largest wave fold %d" % (dname, fold))
        assert 1 << 29 < fold < 1 << 31
        assert fold == 1024 * (960 if dname == "tile_max" else -959) ** 2  # tile_zero: avg = 959, v = -959


# --------------------------------------------------------------------------------------------- 2. LR search
@pytest.mark.parametrize("w,h,bd,rname,sname", ec.LR_CASES)
def test_lr_search_oracle_runs(w, h, bd, rname, sname):
    rec, src, ft, units, recs, out = ec.lr_case(w, h, bd, rname, sname)
    for p in range(3):
        # the RESTORE_NONE cost of a unit is its plain SSE: restated in int64
        us = ec.LR_UNIT_SIZE[p]
        ph, pw = rec[p].shape
        nh, nv = oracle.lr_units(us, pw), oracle.lr_units(us, ph)
        d2 = (rec[p].astype(np.int64) - src[p].astype(np.int64)) ** 2
        for u in range(nh * nv):
            off = 8 if p == 0 else 4  # AV1's restoration units sit 8 luma rows above their grid
            y0, x0 = max((u // nh) * us - off, 0), (u % nh) * us
            y1, x1 = (ph if u // nh == nv - 1 else (u // nh + 1) * us - off), (pw if u % nh == nh - 1 else x0 + us)
            assert recs[p]["sse"][u, 0] == d2[y0:y1, x0:x1].sum(), (p, u)
        evaluated = recs[p]["sse"][:, 1] != ec.I64_MAX
        if (rname, sname) in ec.LR_NEED_WIENER:
            assert evaluated.any(), "plane %d: no unit with an evaluated Wiener filter" % p
    if (rname, sname) == ("flat", "flat"):  # nothing to gain: no restoration, the frame unchanged
        assert ft == [0, 0, 0]
        assert all(np.array_equal(a, b) for a, b in zip(out, rec))


# --------------------------------------------------------------------------------------------- 3. MD batch
@pytest.mark.parametrize("w,bd,sname,rname", ec.MD_CASES)
def test_md_batch_oracle_vs_numpy(w, bd, sname, rname):
    src, refs, runs = ec.md_case(w, bd, sname, rname)
    maxv = (1 << bd) - 1
    seen = set()
    whole = oracle.MD_SHAPES.index((64, 64))
    o64 = sum(4096 // (a * b) for a, b in oracle.MD_SHAPES[:whole])  # the 64x64 block's index among the 849
    for mv, want in runs:
        got, raw = ec.md_numpy(src, refs[0], bd, mv)
        np.testing.assert_array_equal(want, got)  # all 849 blocks of every SB and reference
        seen |= {tuple(int(x) for x in m) for m in mv.reshape(-1, 2)}
        if sname in ("max", "zero") and rname in ("max", "zero"):
            # a uniform difference of +-maxv wherever the block and the clamped reference land
            assert (raw[..., o64] == 4096 * maxv * maxv).all()  # 10 bit: 4 286 582 784, 8 384 512 below 2^32
            assert (want[:, :, 0, o64] == 4096 * maxv).all()
            assert (want[:, :, 0, 0] == 16 * maxv).all()        # a 4x4 cell's |sum| = 16 368 at 10 bit
            assert not want[:, :, 2].any()                      # variance 0
        if (sname, rname) == ("flat", "flat"):
            assert not want.any()
        if (sname, rname) == ("checker", "anti"):
            for i, r in zip(*np.nonzero((mv == 0).all(axis=2))):
                if w == 64:  # at the origin: SAD at its maximum, sum 0, so variance == sse
                    assert want[i, r, 0, o64] == 4096 * maxv
                    np.testing.assert_array_equal(want[i, r, 1], want[i, r, 2])
    assert seen == set(ec.MD_MVS)


# --------------------------------------------------------------------------------------------- 4. MD / ME shims
@pytest.mark.parametrize("bd", [8, 10])
def test_block_dist_oracle_at_full_magnitude(bd):
    maxv = (1 << bd) - 1
    for w, h in mc.MD_SIZES:
        for a, b in ((maxv, 0), (0, maxv)):
            s, r = np.full((h, w), a), np.full((h, w), b)
            sad, sse, var = oracle.block_dist(s, r, w, h, bd)
            raw = w * h * maxv * maxv
            assert sad == w * h * maxv and var == 0
            assert sse == ((raw + 8) >> 4 if bd > 8 else raw & 0xFFFFFFFF)
            assert oracle.block_sse(s, r, w, h, bd) == raw


# --------------------------------------------------------------------------------------------- 5. ME search
@pytest.mark.parametrize("w,h,saw,sah,sub,kind", ec.ME_CASES)
def test_me_search_oracle_vs_numpy_scan(w, h, saw, sah, sub, kind):
    src, refs, org, sad, mv = ec.me_case(w, h, saw, sah, sub, kind)
    nsad, nmv, ties = ec.me_numpy(src, refs, org, saw, sah, sub)
    np.testing.assert_array_equal(sad, nsad)
    np.testing.assert_array_equal(mv, nmv)
    pack = lambda o: ((int(o[1]) & 0xFFFF) << 16) | (int(o[0]) & 0xFFFF)
    if kind == "flat":  # every position ties at 0: every best MV is the origin
        assert not sad.any() and (ties == saw * sah).all()
        for sb in range(org.shape[0]):
            for r in range(ec.ME_NREF):
                assert (mv[sb, r] == pack(org[sb, r])).all()
    elif kind == "max_zero":  # the largest SAD, the same with the doubled sub-sampled rows; still all positions tie
        assert (sad[:, :, 84] == 1044480).all() and (sad[:, :, :64] == 64 * 255).all() and (ties == saw * sah).all()
    elif kind in ("stripe4", "stripe8"):
        # periodic ties wherever the window lies inside the frame; the clamped border breaks the period for some
        # blocks of these small frames, so the tie is required of some block per reference, not of every block
        assert (ties > 1).any(axis=0).all() and (ties < saw * sah).all()
    elif kind == "edge_tie":
        py = (((mv >> 16).astype(np.int64) - org[:, :, 1:2]) & 0xFFFF)[:, 0]
        px = (((mv & 0xFFFF).astype(np.int64) - org[:, :, 0:1]) & 0xFFFF)[:, 1]
        # some of the 85 blocks have their first minimum at row 1 (wave 1), tied with every later row (wave 0's first
        # is row 4), and some at column 1
        assert (py == 1).any() and (px == 1).any()
    else:
        assert (ties[:, 0] == saw * sah).all()  # the corner sample everywhere
        assert (ties[:, 1] % sah == 0).all() and (ties[:, 1] >= sah).all() and (ties[:, 1] < saw * sah).all()
        assert sad[:, :, 84].all()


# --------------------------------------------------------------------------------------------- 6. CCSO
@pytest.mark.parametrize("w,h,bd,kind", ec.CCSO_CASES)
def test_ccso_oracle_runs(w, h, bd, kind):
    pre, org, rec, (rc, prms, flags, ff), outs, ext = ec.ccso_case(w, h, bd, kind)
    maxv = (1 << bd) - 1
    assert rc == 0
    e = [org[p].astype(np.int64)[:h >> (p > 0), :w >> (p > 0)] - rec[p].astype(np.int64)[:h >> (p > 0), :w >> (p > 0)]
         for p in range(3)]
    if kind == "flat_luma":  # one classifier value: every sample of a workgroup in one bin
        assert np.unique(pre).size == 1 and np.unique(ext).size == 1
    if kind in ("max_zero", "zero_max"):
        assert all((x == (maxv if kind == "max_zero" else -maxv)).all() for x in e)
        assert np.unique(ext).size == 1
        # the bounds of ccso_bins_kernel's LDS cell for the samples one workgroup bins here (<= 64 rows x 256)
        n = min(h, 64) * min(w, 256)
        assert n * maxv * maxv < 1 << 49 and n * (maxv + 4096) < 1 << 32 and n < 1 << 15
    if kind == "checker":
        assert all((np.abs(x) == maxv).all() and (x > 0).any() and (x < 0).any() for x in e)
    for p in range(3):  # the apply clips to the sample range and moves a sample only where the plane is enabled
        pl, out = outs[p]
        assert out.shape == pl.shape and int(out.max()) <= maxv
        if not prms[p].enable:
            np.testing.assert_array_equal(out, pl)


# --------------------------------------------------------------------------------------------- 7. DLF
@pytest.mark.parametrize("w,h,bd,rname,sname", ec.DLF_CASES)
def test_dlf_oracle_runs(w, h, bd, rname, sname):
    rec, src, mi, picked, out = ec.dlf_case(w, h, bd, rname, sname)
    assert all(0 <= v <= 63 for v in picked.levels())
    if rname in ("flat", "max"):  # no step at any edge: no level filters anything, every trial level costs the same
        for lv in ((0, 0, 0, 0), (63, 63, 63, 63)):
            f =oracle.dlf_frame(rec, bd, mi, svtgpu.LfParams.make(*lv))
            assert all(np.array_equal(a, b) for a, b in zip(f, rec))
        assert all(np.array_equal(a, b) for a, b in zip(out, rec))
    if rname == "checker":  # full-swing steps at every edge exceed every filter's limit: nothing may move either
        assert all(int(a.max()) <= (1 << bd) - 1 for a in out)


# --------------------------------------------------------------------------------------------- 8. CDEF pick
@pytest.mark.parametrize("w,h,bd,level,rname,sname", ec.CDEF_CASES)
def test_cdef_pick_oracle_on_tied_content(w, h, bd, level, rname, sname):
    rec, src, (mse, skip, d, v), (prm, fbs), out = ec.cdef_case(w, h, bd, level, rname, sname)
    c = oracle.controls(level)
    nf, end = c.first_pass_fs_num, c.first_pass_fs_num + c.default_second_pass_fs_num
    uv = np.array([(c.default_first_pass_fs_uv[g] if g < nf else c.default_second_pass_fs_uv[g - nf]) != -1
                   for g in range(end)])
    live = skip == 0
    assert live.all()  # no block mask: every filter block is searched
    if rname in ec.CDEF_TIED:
        # no strength moves a sample of a constant plane: equal MSE for every searched strength of a live block (the
        # chroma strengths a level leaves unsearched carry the constant default_mse_uv * 64)
        assert (mse[0][live][:, :end] == mse[0][live][:, :1]).all()
        assert (mse[1][live][:, :end][:, uv] == mse[1][live][:, :1]).all()
        assert (mse[1][live][:, :end][:, ~uv] == 1040400 * 64).all()
        assert (sname == "flat") == (not mse[0].any())
        # every pair ties in the first call (or, under the bias, strength 0 wins): one zero strength, nothing filtered
        assert prm[1:] == (0, (0,), (0,)) and not fbs.any()
        assert all(np.array_equal(a, b) for a, b in zip(out, rec))
    if level >= 2:
        assert not uv.all() and uv[:nf].all()
    # the restated pick agrees on these tables too
    import cdef_pick_cases as pc
    rprm, rfbs = pc.finish_cdef_search(mse, skip, c, ec.CDEF_Q, ec.CDEF_LAMBDA)
    assert rprm == prm
    np.testing.assert_array_equal(rfbs, fbs)
