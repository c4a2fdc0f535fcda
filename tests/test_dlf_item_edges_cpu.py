"""The grids of tests/dlf_item_cases.py checked on the CPU alone (Python and the C oracle, no GPU): the hand-laid
superblocks hold the edges they promise, and the oracle agrees with itself on them -- the planes filtered one at a time
equal the planes filtered together, an all-zero level set leaves the picture alone, and the filtered picture differs
from the input along both tile boundaries."""
import numpy as np
import pytest

import dlf_item_cases as ic
import oracle
import synth


@pytest.mark.parametrize("w,h,bd", ic.SHAPES)
def test_item_grids_on_the_oracle(w, h, bd):
    mi = ic.mode_info(w, h, 7)
    for (vert, x, y), want in ic.LUMA_EDGES.items():
        if x < w and y < h:
            assert ic.luma_edge_length(mi, vert, x, y) == want, (vert, x, y)
    assert {ic.luma_edge_length(mi, 0, x, 64) for x in range(0, 128, 4)} == {4, 8, 14}
    assert {ic.luma_edge_length(mi, 1, 64, y) for y in range(0, 64, 4)} == {4, 8, 14}
    _, rec = synth.frame_pair(w, h, bd, seed=0x5EED0400 + bd)
    prm = ic.params((40, 36, 20, 28))
    both = oracle.dlf_frame(rec, bd, mi, prm)
    for p in range(3):
        one = oracle.dlf_frame(rec, bd, mi, prm, p, p + 1)
        assert np.array_equal(one[p], both[p]), p
        assert all(np.array_equal(one[k], rec[k]) for k in range(3) if k != p), p
    # both tile boundaries are filtered (luma rows / columns 56..71 around 64), the level-0 class on one side included
    d = both[0].astype(np.int64) - rec[0].astype(np.int64)
    assert d[:16, 60:68].any() and d[60:68, :].any() and d[:, 60:68].any()
    zero = oracle.dlf_frame(rec, bd, mi, ic.params((0, 0, 0, 0)))
    assert all(np.array_equal(a, b) for a, b in zip(zero, rec))
