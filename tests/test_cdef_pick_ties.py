"""CPU half of the CDEF pick's tie, boundary and large-frame cases (cdef_pick_cases.py): the oracle's pick equals a
plain restatement of finish_cdef_search on every case the restatement can afford, the restatement's
svt_search_one_dual equals the reference's on the tie golden, and every case reaches the tie, the width or the live
count it is built for.  The device is held to the same oracle results in test_cdef_pick_ties_gpu.py."""
import numpy as np
import pytest

import cdef_cases as cc
import cdef_pick_cases as pc
import oracle


def _calls(trace):
    return [t for t in trace if "tot" in t]


@pytest.mark.parametrize("key", pc.RESTATED, ids=pc.case_id)
def test_oracle_pick_equals_restatement(key):
    c = pc.case(key)
    (prm, fbs), trace = c.restated()
    oprm, ofbs = c.want()
    assert oprm == prm
    np.testing.assert_array_equal(ofbs, fbs)
    assert not ofbs[c.skip != 0].any()
    assert len(_calls(trace)) == 75  # 5 + 10 + 20 + 40 calls of svt_search_one_dual


def test_restated_search_one_dual_equals_reference_on_ties():
    """The restatement's svt_search_one_dual against the reference's own, on the tie golden."""
    g = cc.load("cdef_search_one_dual_ties.bin")
    for n in range(len(g["best"])):
        nb, start, end = (int(x) for x in g["params"][n])
        sb = int(g["sb"][n])
        l0, l1 = [int(x) for x in g["lev_in"][n][0]], [int(x) for x in g["lev_in"][n][1]]
        m = g["mse"][n].astype(np.uint64)
        best = pc.search_one_dual(l0, l1, nb, m[0, :sb], m[1, :sb], start, end)
        assert best == int(g["best"][n]), n
        assert l0 == list(g["lev_out"][n][0]) and l1 == list(g["lev_out"][n][1]), n


def test_tie_golden_rows_are_the_families():
    """The golden's rows are the rows of cdef_pick_cases' families (population = block index mod populations), and
    every case has at least two minimal pairs, so its result depends on the first-minimum rule."""
    g = cc.load("cdef_search_one_dual_ties.bin")
    names = ("const", "mod", "lane", "two")
    assert set(int(f) for f in g["family"]) == {0, 1, 2, 3}
    assert set(int(p[0]) for p in g["params"]) == set(range(8))
    assert {int(p[1]) for p in g["params"]} == {0, 3} and {int(p[2]) for p in g["params"]} == {64, 48, 4}
    for n in range(len(g["best"])):
        fam, sb = names[int(g["family"][n])], int(g["sb"][n])
        assert 1 <= sb <= 16
        for i in range(sb):
            m0, m1 = pc.family_rows(fam, int(g["arg"][n]), i % pc.POPULATIONS[fam])
            np.testing.assert_array_equal(g["mse"][n][0, i], m0.astype(np.uint64))
            np.testing.assert_array_equal(g["mse"][n][1, i], m1.astype(np.uint64))
        nb, start, end = (int(x) for x in g["params"][n])
        trace = []
        m = g["mse"][n].astype(np.uint64)
        pc.search_one_dual([int(x) for x in g["lev_in"][n][0]], [int(x) for x in g["lev_in"][n][1]], nb, m[0, :sb],
                           m[1, :sb], start, end, trace)
        assert len(pc.minimal_pairs(trace[0])) >= 2, n


# ------------------------------------------------------------------------------------------------ reach
@pytest.mark.parametrize("key", [k for k in pc.RESTATED if k[0] == "lane" and pc.case(k).live > 0], ids=pc.case_id)
def test_lane_first_minimum_is_not_in_the_lowest_lane(key):
    """e = 323 (lane 323 % 256 = 67: wave 1 of a 256-thread workgroup) is the first minimum and ties with e = 515
    (lane 3, wave 0): a fold that prefers the lower lane or wave over the lower index picks (8, 3), not (5, 3)."""
    (prm, _), trace = pc.case(key).restated()
    first = _calls(trace)[0]
    e = pc.minimal_pairs(first)
    assert e == [323, 328, 515, 520] and first["pick"] == (5, 3)
    assert any(x % 256 < e[0] % 256 for x in e[1:])
    assert prm[2][0] == 4 * 5 and prm[3][0] == 4 * 3  # level 1: strength index g of the first pass has code 4 g


@pytest.mark.parametrize("key", [k for k in pc.RESTATED if k[0] == "const"], ids=pc.case_id)
def test_const_every_pair_of_every_call_ties(key):
    c = pc.case(key)
    (prm, fbs), trace = c.restated()
    calls = _calls(trace)
    end = calls[0]["end"]
    bias = oracle.controls(c.level).zero_fs_cost_bias
    for n, call in enumerate(calls):
        if bias and call["nb_sel"] == 0:
            # the biased (0, 0) is the single minimum where nothing is selected yet; once it is, every block's best is
            # its (0, 0) and every pair ties again
            assert pc.minimal_pairs(call) == [0], n
        else:
            assert len(pc.minimal_pairs(call)) == end * end, n
        assert call["pick"] == (0, 0), n
    assert prm[1] == 0 and prm[2] == (0,) and prm[3] == (0,) and not fbs.any()
    if c.lam == 0:  # the four strength counts cost the same: the strict < keeps one strength
        costs = [t["cost"] for t in trace if "cost" in t]
        assert len(costs) == 4 and len(set(costs)) == 1


@pytest.mark.parametrize("key", [k for k in pc.RESTATED if k[0] in ("two", "four")], ids=pc.case_id)
def test_populations_signal_their_strengths(key):
    c = pc.case(key)
    (prm, fbs), trace = c.restated()
    npop = pc.POPULATIONS[c.family]
    if c.live >= npop:
        assert prm[1] == {2: 1, 4: 2}[npop]
        live = np.nonzero(c.skip == 0)[0]
        for r in range(npop):  # one strength index per population
            assert len(set(fbs[live[live % npop == r]].tolist())) == 1
        assert len(set(fbs[live].tolist())) == npop
    if c.family == "two" and c.live % 2 == 0 and c.live and _calls(trace)[0]["end"] >= 8:
        # equally many blocks of either population: their optima tie in the first call (levels that search at least
        # one period of the rows: the 4 strengths of levels 9 and 12 have a single minimum)
        assert len(pc.minimal_pairs(_calls(trace)[0])) >= 2


@pytest.mark.parametrize("key", [k for k in pc.FB_TIES if k[0] == "tie3"], ids=pc.case_id)
def test_tie3_blocks_tie_between_the_signalled_strengths(key):
    """More than one strength is signalled and a third of the live blocks cost the same under each of them: the
    reference's strict < gives them index 0 (a <= in the per-FB assignment gives them the last index)."""
    c = pc.case(key)
    prm, fbs = c.want()
    assert prm[1] >= 1 and len(set(zip(prm[2], prm[3]))) == 1 << prm[1]
    live = np.nonzero(c.skip == 0)[0]
    flat = live[live % 3 == 2]
    assert len(flat) >= 1 and (c.mse[:, flat] == pc.D_POP).all() and not fbs[flat].any()
    assert fbs[live].max() >= 1
    if key in pc.RESTATED:
        assert c.restated()[0][0] == prm


def test_wide_lane_sums_straddle_32_bits():
    """Every entry is >= 2^31 - 10: the minimal sums are 2^32 - 10 and all others exactly 2^32, which a 32-bit sum
    wraps to 0.  The first minimal pair is (5, 0)."""
    for key in (k for k in pc.FB_TIES if k[0] == "wide_lane"):
        c = pc.case(key)
        (prm, _), trace = c.restated()
        first = _calls(trace)[0]
        sums = c.mse[0, 0, :first["end"], None].astype(object) + c.mse[1, 0, None, :first["end"]].astype(object)
        assert set(sums.ravel().tolist()) == {(1 << 32) - 10, 1 << 32}
        assert first["pick"] == (5, 0) and pc.minimal_pairs(first)[0] == 5 * 64 and (c.mse >= pc.W31).any()
        assert prm == c.want()[0]


def test_width_cases_sit_on_the_flag():
    """pick_gather_kernel selects the 64-bit accumulation when an entry (after the zero-strength bias) is >= 2^31."""
    for key in pc.WIDE + pc.UHD[1:3]:
        c = pc.case(key)
        wide = int((c.mse >= pc.W31).sum())
        if c.family == "one_wide":
            assert wide == 1
            p, g = c.arg
            fb = np.nonzero(c.skip == 0)[0][-1]
            assert c.mse[p, fb, g] == pc.W31
            ctr = oracle.controls(c.level)
            if g:  # past the searched strengths: no call reads the entry that raises the flag
                assert g >= ctr.first_pass_fs_num + ctr.default_second_pass_fs_num
        elif c.arg == pc.W31 - 1:
            assert wide == 0 and int(c.mse.max()) * 2 == (1 << 32) - 2  # m0 + m1 one below the 32-bit best's clamp
        else:
            assert c.arg == pc.W31 and wide == c.mse.size
            bias = oracle.controls(c.level).zero_fs_cost_bias
            if c.level == 12:  # entry 0 comes back under 2^31, the others stay wide
                assert bias == 62 and (bias * pc.W31) >> 6 < pc.W31
    assert any(k[0] == "const" and k[1] == pc.W31 and k[4] == 12 for k in pc.WIDE)


def test_chunk_cases_live_counts():
    """The live FBs are the frame's last 32, 33 (four chains: chunks of 32), 8 and 9 (one chain: chunks of 8), behind
    more than 256 skipped ones; the single-FB cases cover the first FB and the last."""
    seen = set()
    for key in pc.CHUNK:
        c = pc.case(key)
        assert c.nfb == 510 and c.live == key[6][1]
        assert np.nonzero(c.skip == 0)[0][0] == 510 - c.live > 256
        seen.add(c.live)
    assert seen == set(pc.CHUNK_LIVE)
    assert {int(np.nonzero(pc.case(k).skip == 0)[0][0]) for k in pc.SINGLE} == {0, 509}
    assert all(pc.case(k).live == 1 for k in pc.SINGLE)
    assert [pc.nfb_of(k[2], k[3]) for k in pc.TINY[::4]] == [1, 2, 3, 5, 65]
    assert {pc.nfb_of(k[2], k[3]) for k in pc.LARGE} == {2304, 8160} and pc.nfb_of(3840, 2160) == 2040
    assert all(pc.case(k).live == 33 for k in pc.LARGE if k[0] == "two")


def test_mod_first_minimum_is_not_at_index_zero():
    for key in (k for k in pc.RESTATED if k[0] == "mod"):
        _, trace = pc.case(key).restated()
        first = _calls(trace)[0]
        assert first["pick"] != (0, 0)
        if first["end"] >= 8:  # at least one period of the rows is searched (levels 1, 2 and 5)
            assert len(pc.minimal_pairs(first)) >= 2


def test_levels_cover_the_strength_counts():
    ends = {lv: oracle.controls(lv).first_pass_fs_num + oracle.controls(lv).default_second_pass_fs_num
            for lv in (1, 2, 5, 9, 12)}
    assert ends == {1: 64, 2: 48, 5: 16, 9: 4, 12: 4}
    assert {k[4] for k in pc.LEVELS} == set(ends)
