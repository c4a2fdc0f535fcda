"""The temporal filter's restatements on worst-case and all-tie content, without a GPU: tf_search_cases.search_frame,
err32_of_use64, interp_cases.predict_frame and tf_cases.filter_frame against every record the reference's C left in
tests/golden/tf_extreme.bin, bit for bit, and, on the restatement, that each case reaches what it is there for.

Three things the contents turned out to be, against what was first written down for them:
  * inv_checker_walk is a checker of 2 x 2 cells against its inverse.  On the plain (x + y) & 1 checker no convolve form
    ever leaves the sample range (the taps of an alternating 0 / max row nearly cancel), so no clip acts; on cells of two
    samples every form overshoots.  inv_checker_pinned and th32_wide keep the plain checker: they evaluate the start only.
  * inv_checker_pinned is unsplit, with the stated errors, in the 32x32 blocks at x <= 96, y <= 32 only.  Beyond them the
    MV clamp of a block that starts more than 3 samples past the 136 x 72 picture moves the zero MV by a whole number of
    samples; an odd move turns the inverse checker into the centre, the error of that sub-block is 0, and its parent splits.
  * v_stripes / h_stripes cannot tell the reference's "x outer, y inner" order from "y outer, x inner": the positions that
    tie differ along the stripes only, and both orders meet the -1 of that axis before its 0 and +1, so both keep the same
    first of the tied positions.  What they pin down is the strict <: the first of the tied positions stays (asserted).
    The order is decided where two positions tie that are each other's transpose, which inv_checker_walk has at every
    block ((-4, 0) against (0, -4)): the transposed walk is asserted to end elsewhere there.
near_max is a case added to those first written down: inv_checker_pinned brings the four-wave combine its largest sse, but
its 64x64 error fails the 64-vs-32 test whether or not the combine is right; on near_max that error decides use64."""
import functools

import numpy as np
import pytest

import interp_cases as ic
import tf_cases as fc
import tf_extreme_cases as xc
import tf_search_cases as tc

CASES = xc.search_cases()
CHAINS = xc.chain_cases()
FILTERS = xc.filter_cases()
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _walk(i):
    """(records, trace) of search case i from the restatement, computed once."""
    c, trace = CASES[i], []
    if c["cls"] == "inv_checker_walk":
        c = dict(c, P=dict(c["P"], trace_clip=True))
    return tc.search_frame(c, trace=trace), trace


def _runs(trace):
    """The trace split into searches: consecutive positions of one block."""
    out = []
    for e in trace:
        if out and (out[-1][0]["b"], out[-1][0]["px"], out[-1][0]["py"]) == (e["b"], e["px"], e["py"]) and len(out[-1]) < 25:
            out[-1].append(e)
        else:
            out.append([e])
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_search_restatement_matches_the_record(i):
    got, _ = _walk(i)
    for f in tc.FIELDS:
        np.testing.assert_array_equal(got[f], CASES[i]["want"][f], err_msg="%s %s" % (CASES[i]["name"], f))


@pytest.mark.parametrize("c", CHAINS, ids=[c["name"] for c in CHAINS])
def test_chain_restatements_match_the_record(c):
    """search_frame, err32_of_use64 on the recorded predictors, predict_frame on the recorded motion, filter_frame on the
    recorded predictors and patched blocks."""
    got = tc.search_frame(c)
    for f in tc.FIELDS:
        np.testing.assert_array_equal(got[f], c["want"][f], err_msg="%s %s" % (c["name"], f))
    pics, bd = c["pics"], c["pic_bd"]
    e32 = tc.err32_of_use64(c["want"], [p[0] for p in c["pred"]], pics["cen"][0], bd, c["P"]["shift"])
    np.testing.assert_array_equal(e32, c["err32p"])
    assert c["want"]["use64"][0, 1] and c["want"]["use64"][1, 4]  # the forced blocks: err32 of a full-range 32x32
    motion = tc.motion_dicts(tc.motion_block_arrays(c["want"])[0])
    for r in range(c["n_refs"]):
        pred = ic.predict_frame(pics["ref"][r], c["pad"], motion[r], bd, tc.W, tc.H, 1)
        for p in range(3):
            np.testing.assert_array_equal(pred[p], c["pred"][r][p], err_msg="%s reference %d plane %d" % (c["name"], r, p))
    out = fc.filter_frame(pics["cen"], c["pred"], xc.block_metas(c["want"], c["err32p"]), c["decay"], c["mv_dist_th"], 1, bd, 0,
                          tc.W, tc.H)
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(out[p][:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))


def test_chain_err32_is_the_full_range_one():
    """max_zero at 8 bits: a forced block's 32x32 quadrants differ by 255 everywhere: sum = 261 120, sum^2 = 6.8e10 beyond
    32 bits, and the variance is exactly 0."""
    c = CHAINS[0]
    assert c["cls"] == "max_zero" and c["pic_bd"] == 8
    d = c["pred"][0][0][:32, 64:96].astype(np.int64) - c["pics"]["cen"][0][:32, 64:96]
    assert abs(int(d.sum())) == 261120 and int(d.sum()) ** 2 > 1 << 32 and (c["err32p"][0, 1] == 0).all()


def _of(cls):
    return [i for i, c in enumerate(CASES) if c["cls"] == cls]


def test_fixture_holds_the_cases():
    assert [c["cls"] for c in CASES].count("inv_checker_walk") == 16 and len(CASES) == 30
    for cls in xc.CLASSES:
        assert {CASES[i]["P"]["bd"] for i in _of(cls)} == {8, 10}, cls
    for bd in (8, 10):  # every value of every switch, and every pair of values of two switches
        rows = {(c["P"]["modes"], c["P"]["use_2tap"], c["P"]["shift"], c["P"]["enable8"]) for c in CASES
                if c["cls"] == "inv_checker_walk" and c["P"]["bd"] == bd}
        assert len(rows) == 8 and {r[0] for r in rows} == {(1, 1, 1), (2, 2, 2)}
        for a in range(4):
            for b in range(a + 1, 4):
                assert len({(r[a], r[b]) for r in rows}) == 4
    assert [(c["cls"], c["pic_bd"], c["P"]["bd"]) for c in CHAINS] == [("max_zero", 8, 8), ("inv_checker_walk", 10, 10)]


def test_max_zero_reaches_its_point():
    for i in _of("max_zero"):
        c, (rec, trace) = CASES[i], _walk(i)
        assert all(e["dist"] == 0 for e in trace) and not rec["err32"].any() and not rec["err16"].any()
        assert rec["split32"].all() and rec["split16"].all() and not rec["use64"].any()
        assert all(len(r) == 1 for r in _runs(trace))  # best == 0 after the first position: nothing else is evaluated
        big = [e for e in trace if e["b"] == 64]
        if c["P"]["bd"] == 8:  # reference 0: 4096 samples that differ by 255
            assert max(e["sum"] ** 2 for e in big) == (4096 * 255) ** 2 > 1 << 32
        else:  # (sum + 2) >> 2 squared
            assert max(((e["sum"] + 2) >> 2) ** 2 for e in big) > 1 << 32


def test_inv_checker_pinned_reaches_its_point():
    for i in _of("inv_checker_pinned"):
        c, (rec, trace) = CASES[i], _walk(i)
        bd = c["P"]["bd"]
        e32 = 66977856 if bd > 8 else 66585600
        assert not rec["use64"].any() and all(len(r) == 1 for r in _runs(trace))
        for blk in range(tc.NBLK):
            for q in range(4):
                if (blk % 3) * 64 + (q & 1) * 32 <= 96 and (blk // 3) * 64 + (q >> 1) * 32 <= 32:
                    assert not rec["split32"][:, blk, q].any() and (rec["err32"][:, blk, q] == e32).all(), (blk, q)
        e64 = max(e["dist"] for e in trace if e["b"] == 64)
        sse = max(e["sse"] for e in trace if e["b"] == 64)
        assert sse == 4096 * ((1 << bd) - 1) ** 2 and (1 << 31 < sse < 1 << 32) == (bd > 8)  # 4 286 582 784 at 10 bits
        assert e64 == 4 * e32 and e64 * 14 > 1 << 31  # 3.75e9 against 4.29e9: both sides of the 64-vs-32 test pass 2^31
        assert e64 * 14 < 4 * e32 * 16 and not e64 < 1 << 18  # and the test fails on its second half alone


def test_inv_checker_walk_reaches_its_point():
    kinds = {}
    for i in _of("inv_checker_walk"):
        c, (rec, trace) = CASES[i], _walk(i)
        for e in trace:
            k = (c["P"]["bd"], e["form"])
            kinds[k] = kinds.get(k, 0) + e["clipped"]
        forms = (1, 2, 3) if c["P"]["modes"][0] == 1 else (1, 2)  # mode 2 has no diagonal position
        for f in forms:
            assert any(e["clipped"] for e in trace if e["form"] == f), (c["name"], f)
        assert rec["mv64"].any() or rec["mv32"].any() or rec["mv16"].any() or rec["mv8"].any(), c["name"]  # the starts are 0
        if not c["P"]["shift"]:  # with every second row left out x and y are no longer each other's transpose
            alt = tc.search_frame(c, y_outer=True)
            assert any((alt[f] != rec[f]).any() for f in ("mv64", "mv32", "mv16", "mv8")), c["name"]
    assert all(kinds[(bd, f)] > 0 for bd in (8, 10) for f in (1, 2, 3)), kinds


def test_flat_ref_reaches_its_point():
    for i in _of("flat_ref"):
        c, (rec, trace) = CASES[i], _walk(i)
        for r in _runs(trace):
            assert len(r) == 25 and r[0]["dist"] > 0 and all(e["dist"] == r[0]["dist"] for e in r)
        fp, u = c["fullpel"], rec["use64"].astype(bool)
        assert not u.any()
        s32, s16 = rec["split32"].astype(bool), rec["split16"].astype(bool)
        np.testing.assert_array_equal(rec["mv32"][~s32], 8 * fp["mv32"][~s32])
        np.testing.assert_array_equal(rec["bmv16"][np.repeat(s32, 4, axis=-1)], 8 * fp["mv16"][np.repeat(s32, 4, axis=-1)])
        np.testing.assert_array_equal(rec["mv8"][np.repeat(s16, 4, axis=-1)], 8 * fp["mv8"][np.repeat(s16, 4, axis=-1)])
        assert s32.any()


@pytest.mark.parametrize("cls", ["v_stripes", "h_stripes"])
def test_stripes_reach_their_point(cls):
    """Positions that differ along the stripes only tie, the walk moves across them, and of the tied positions the first
    one evaluated stays: the component along the stripes of every MV that moved is -(4 + 2 + 1)."""
    along = 1 if cls == "v_stripes" else 0
    for i in _of(cls):
        c, (rec, trace) = CASES[i], _walk(i)
        moved, graded = 0, 0
        for r in _runs(trace):
            by = {}
            for e in r:
                by.setdefault(e["mv"][1 - along], set()).add(e["dist"])
            assert all(len(v) == 1 for v in by.values()) and len(r) == 25 and r[0]["dist"] > 0
            graded += len(set.union(*by.values())) > 1
        assert graded  # across the stripes the error changes (but in blocks the MV clamp moves past the picture)
        for f in ("mv32", "mv16", "mv8"):
            m = rec[f].reshape(-1, 2)
            m = m[m.any(axis=1)]
            moved += len(m)
            assert (m[:, along] == -7).all(), (c["name"], f)
        assert moved


def test_th32_wide_reaches_its_point():
    for i in _of("th32_wide"):
        c, (rec, _) = CASES[i], _walk(i)
        assert c["P"]["th32"] == 1 << 32 and not rec["split32"].any() and rec["err32"].max() > 0
        narrow = tc.search_frame(dict(c, P=dict(c["P"], th32=c["P"]["th32"] & M32)))
        assert narrow["split32"].any() and any((narrow[f] != rec[f]).any() for f in tc.FIELDS)


def test_near_max_reaches_its_point():
    """The 64x64 error decides use64, and at 10 bits it comes from an sse in (2^31, 2^32): every block ends on the 64x64
    path; the same moments combined in a signed 32-bit sse give an error of some 4e9 and no block does."""
    for i in _of("near_max"):
        c, (rec, trace) = CASES[i], _walk(i)
        bd = c["P"]["bd"]
        big = [e for e in trace if e["b"] == 64]
        assert rec["use64"].all() and len(big) == tc.NR * tc.NBLK and not rec["mv64"].any()
        e64, e32 = (64, 16) if bd > 8 else (1024, 256)
        assert {e["dist"] for e in big} == {e64} and {e["dist"] for e in trace if e["b"] == 32} == {e32}
        assert e64 * 14 < 4 * e32 * 16 and e64 < 1 << 18
        if bd > 8:
            sse, sm = big[0]["sse"], big[0]["sum"]
            assert (sse, -sm) == (4282394624, 4188160) and 1 << 31 < sse < 1 << 32
            wrapped = ((sse - (1 << 32) + 8) >> 4) & M32  # the sse as a signed 32-bit value, widened, in the same formula
            assert not max(wrapped - ((sm + 2) >> 2) ** 2 // 4096, 0) < 1 << 18


@pytest.mark.parametrize("c", FILTERS, ids=[c["name"] for c in FILTERS])
def test_filter_restatement_matches_the_record(c):
    """The output, and every quadrant's weight and whether its avg_err product passes 2^32, in the walk's order."""
    stats = []
    out = fc.filter_frame(c["centre"], c["refs"], c["metas"], c["decay"], c["mv_dist_th"], 1, c["bd"], 0, c["w"], c["h"], stats)
    for p in range(3):
        hh, ww = c["out"][p].shape
        np.testing.assert_array_equal(out[p][:hh, :ww], c["out"][p], err_msg="%s plane %d" % (c["name"], p))
    np.testing.assert_array_equal(np.array([w for _, w, _ in stats]), c["wt"].reshape(-1))
    np.testing.assert_array_equal(np.array([int(wide) for _, _, wide in stats]), c["wide"].reshape(-1))
    wt, wide = c["wt"].reshape(-1, 3, 4), c["wide"].reshape(-1, 3, 4)
    for k, planes in enumerate((slice(0, 1), slice(1, 3))):
        occ = [(wt[:, planes] == 1000).sum(), (wt[:, planes] == 0).sum(), ((wt[:, planes] > 0) & (wt[:, planes] < 1000)).sum(),
               wide[:, planes].sum()]
        assert occ == [int(v) for v in c["occ"][k]]
        if c["name"] == "wide_frame":
            assert min(occ) > 0, (k, occ)
        else:
            assert occ[0] == occ[1] == 13 * 16 * (1 + k) and occ[2] == 0


def test_wide_frame_meets_the_wraps():
    c = FILTERS[0]
    mv = np.concatenate([c["metas"][2][b][f].reshape(-1, 2) for b in range(c["nblk"]) for f in ("mv32", "mv16")]).astype(np.int64)
    assert (np.abs(mv) == 16383).all() and ((mv ** 2).sum(axis=1) << 8).min() > M32  # (col^2 + row^2) << 8 wraps
    ds = {fc.d_factor_fp8(int(x), int(y), c["mv_dist_th"]) for x, y in np.concatenate(
        [c["metas"][1][b][f].reshape(-1, 2) for b in range(c["nblk"]) for f in ("mv32", "mv16")])}
    assert min(ds) >= 17000 and max(ds) < 100000  # d_factor in the tens of thousands on the full-range reference


def test_refs26_reaches_its_point():
    for c in FILTERS[1:]:
        assert c["n_refs"] == 26 and (c["w"], c["h"], c["nblk"]) == (64, 64, 1)
        wt = c["wt"].reshape(26, 4, 3, 4)
        assert (wt[0::2] == 1000).all() and (wt[1::2] == 0).all()  # count = 1000 + 13 * 1000 >= 14 000
        for p in range(3):
            np.testing.assert_array_equal(c["out"][p], c["centre"][p])
