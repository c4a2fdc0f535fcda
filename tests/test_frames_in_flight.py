"""The frame groups of tests/pipeline_cases.GROUPS, from the goldens alone (CPU): a stage state that kept a decision
of the frame before -- levels, CDEF parameters or per-block strengths, LR units, or a whole output picture -- cannot
pass tests/test_frames_in_flight_gpu.py, because every two frames that follow one another in a group's sequence differ
in each of them.  The sequences wrap around (A, B, C, A, B), so the pairs are the cyclic ones."""
import numpy as np
import pytest

import pipeline_cases as pc

PAIRS = [(g, names[i], names[(i + 1) % len(names)]) for g, names in pc.GROUPS.items() for i in range(len(names))
         if len(names) > 2 or i == 0]


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_group_shares_one_state(group):
    """One DlfState / CdefState / LrState serves the whole group: equal picture size, bit depth and LR unit sizes."""
    cs = [pc.CASES[n] for n in pc.GROUPS[group]]
    assert len({(c["w"], c["h"], c["bd"], c["us"], c["sb"], c["digest"]) for c in cs}) == 1
    assert len(set(pc.GROUPS[group])) == len(cs) >= 2


@pytest.mark.parametrize("group,a,b", PAIRS)
def test_consecutive_frames_differ_in_every_decision(group, a, b):
    ga, gb = pc.load(a), pc.load(b)
    assert tuple(ga["lf_levels"]) != tuple(gb["lf_levels"]), "DLF levels"
    assert list(ga["cdef_params"]) != list(gb["cdef_params"]), "cdef_params"
    assert not np.array_equal(ga["cdef_fbs"], gb["cdef_fbs"]), "cdef_fbs"
    assert any(not np.array_equal(ga["lr_units%d" % p], gb["lr_units%d" % p]) for p in range(3)), "LR units"
    for key in ("dlf", "cdef", "lr"):
        for p in range(3):
            assert not np.array_equal(ga["%s%d" % (key, p)], gb["%s%d" % (key, p)]), "%s plane %d" % (key, p)


@pytest.mark.parametrize("group", list(pc.GROUPS))
def test_group_signals_two_strength_counts(group):
    """cdef_bits (cdef_params[1]) takes at least two values: the apply's strength table changes length in a group."""
    assert len({int(pc.load(n)["cdef_params"][1]) for n in pc.GROUPS[group]}) >= 2


def test_new_cases_take_the_paths_the_groups_need():
    """The 8-bit group's third case runs the device level search (a DLF level that is not SB-based) and a searched
    CDEF level; the 320x200 group's new cases use CDEF levels with different strength counts, one low and one high
    share of skipped blocks."""
    import pipeline_run as pr
    c = pc.CASES["seq8_c"]
    assert not pr.dlf_ctrls(c["dlf_level"])["sb_based"] and not pr.cdef_ctrl_row(c["cdef_level"])["ref_fs"]
    counts = [sum(pr.cdef_ctrl_row(pc.CASES[n]["cdef_level"])[k] for k in ("n1", "n2")) for n in pc.GROUPS["320x200_10"]]
    assert len(set(counts)) == 3, counts
    shares = sorted(pc.CASES[n]["mi"][2] for n in ("seq10_b", "seq10_c"))
    assert shares[0] <= 0.1 and shares[1] >= 0.6
