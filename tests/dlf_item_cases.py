"""Mode-info grids for the deblocking tile item's edge cases (tests/test_dlf_item_edges_gpu.py and its CPU check).

The four superblocks around the tile corner (64, 64) are laid out by hand on top of a random valid partition, so that
the edges the item's apron trimming and packed write-back depend on exist at known places:
  * 14-tap luma edges on the tile boundaries x = 64 and y = 64 (64x64, 64x16, 16x64 and 16x16 transforms on both sides),
    which are the edge at y0 / x0 of the second tile row / column and the edge at y0+64 / x0+64 of the first;
  * lengths 4, 8 and 14 (chroma: 4 and 6) in neighbouring 4-sample segments along both boundaries;
  * 4x4 blocks next to the boundaries: edges at 60 and 68, the item's outermost edge rows / columns (y0-4, y0+68).  An
    edge record takes a length above 4 only at a coordinate that is a multiple of 8 (8) or 16 (14) -- the transform
    edge must lie on the transform grid -- so with tile origins on the 64 grid those two rows can hold 4-tap edges only:
    a 14-tap edge at y0-4 or y0+68 cannot be built from any grid;
  * runs of 8x8 transforms: length-8 edges with length-8 neighbours 8 samples away on both sides;
  * one 64x16 block of reference frame 2, whose level class the parameters' reference delta takes to level 0: an edge
    with level 0 on one side.
"""
import numpy as np

import dlf_cases as dc
from svtgpu import LF_MI_DTYPE, LfParams

SHAPES = [(136, 72, 8), (200, 136, 10)]  # two tile columns and rows, a partial last tile, chroma widths 68 / 100
REF_DELTAS = (1, 0, -63, 0, -1, 0, -1, -1)  # reference frame 2: level 0 at every base level


def params(levels):
    return LfParams.make(*levels, ref_deltas=REF_DELTAS, mode_deltas=(0, 0))


def blocks():
    """(x, y, w, h, tx_depth, ref_frame) of the hand-laid superblocks (0..127 x 0..127), in samples."""
    out = [(0, 0, 64, 64, 0, 1)]                                      # SB (0, 0): one 64x64 transform
    # SB (1, 0): right of x = 64, above y = 64
    out += [(64, 0, 64, 16, 0, 2)]                                    # 64x16, level class 0: 14-tap at x = 64
    out += [(x, y, 8, 8, 0, 1) for y in (16, 24) for x in range(64, 128, 8) if (x, y) != (64, 24)]
    out += [(x, y, 4, 4, 0, 1) for y in (24, 28) for x in (64, 68)]   # 4-tap at x = 64 and 68
    out += [(x, 32, 16, 16, 0, 1) for x in range(64, 128, 16)]        # 14-tap at x = 64, 80, 96, 112
    out += [(64, 48, 16, 16, 0, 1)]                                   # 16 tall above y = 64
    out += [(80, 48, 8, 8, 0, 1), (80, 56, 8, 8, 0, 1), (88, 48, 8, 8, 0, 1)]
    out += [(x, y, 4, 4, 0, 1) for y in (56, 60) for x in (88, 92)]   # edges at y = 60 and 64, 4-tap
    out += [(96, 48, 16, 16, 0, 1), (112, 48, 16, 16, 1, 1)]          # 16 tall; 8x8 transforms
    # SB (0, 1): left of x = 64, below y = 64
    out += [(0, 64, 16, 64, 0, 1)]                                    # 16x64: 14-tap at y = 64
    out += [(x, y, 8, 8, 0, 1) for x in range(16, 32, 8) for y in range(64, 128, 8)]
    out += [(x, y, 4, 4, 0, 1) for y in (64, 68) for x in range(32, 48, 4)]  # 4-tap at y = 64 and 68
    out += [(x, y, 8, 8, 0, 1) for x in range(32, 48, 8) for y in range(72, 128, 8)]
    out += [(48, 64, 16, 16, 0, 1)]                                   # 14-tap at y = 64 and at x = 64
    out += [(x, y, 4, 4, 0, 1) for y in range(80, 96, 4) for x in range(48, 64, 4)]  # 4-tap at x = 52, 56, 60, 64
    out += [(x, y, 8, 8, 0, 1) for x in (48, 56) for y in range(96, 128, 8)]
    # SB (1, 1)
    out += [(64, 64, 16, 64, 0, 1)]                                   # 16x64 right of x = 64, below y = 64
    out += [(x, y, 8, 8, 0, 1) for x in (80, 88) for y in range(64, 128, 8)]
    out += [(96, 64, 16, 16, 0, 1)]
    out += [(x, y, 8, 8, 0, 1) for x in (96, 104) for y in range(80, 128, 8)]
    out += [(x, y, 4, 4, 0, 1) for y in (64, 68) for x in range(112, 128, 4)]
    out += [(x, y, 8, 8, 0, 1) for x in (112, 120) for y in range(72, 128, 8)]
    return out


def mode_info(width, height, seed):
    mi = dc.random_mode_info(width, height, seed, p_skip=0.3)
    mr, mc = mi.shape
    cover = np.zeros((32, 32), np.int32)
    for x, y, w, h, txd, ref in blocks():
        assert x % w == 0 and y % h == 0, (x, y, w, h)
        cover[y // 4:(y + h) // 4, x // 4:(x + w) // 4] += 1
        if y // 4 < mr and x // 4 < mc:  # a block may reach past the picture; its inside part is listed
            mi[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = (dc._BS[(w, h)], txd, 0, ref, 16, 0, (0, 0))
    assert (cover == 1).all(), "the hand-laid superblocks are a partition"
    return mi


# luma edge lengths the layout promises: (vertical?, x, y) -> length (checked where the picture holds the position)
LUMA_EDGES = {
    (1, 64, 0): 14, (1, 64, 16): 8, (1, 64, 24): 4, (1, 68, 24): 4, (1, 64, 32): 14, (1, 64, 48): 14,
    (1, 72, 16): 8, (1, 80, 16): 8, (1, 80, 32): 14, (1, 60, 80): 4, (1, 64, 80): 4, (1, 64, 64): 14,
    (0, 0, 64): 14, (0, 16, 64): 8, (0, 24, 64): 8, (0, 32, 64): 4, (0, 32, 68): 4, (0, 48, 64): 14,
    (0, 64, 64): 14, (0, 80, 64): 8, (0, 88, 64): 4, (0, 88, 60): 4, (0, 96, 64): 14, (0, 112, 64): 4,
    (0, 112, 68): 4, (0, 104, 64): 14,
}


def luma_edge_length(mi, vert, x, y):
    """The luma filter length of the edge at (x, y) of the hand-laid region by the rule of the edge records (non-skip
    blocks): 0 off the transform grid, else from the smaller transform across it."""
    def tx(m):
        w, h = dc.BW[int(m["bsize"])], dc.BH[int(m["bsize"])]
        if int(m["tx_depth"]) == 0:
            return (min(w, 64), min(h, 64))
        assert w == h == 16 and int(m["tx_depth"]) == 1, "the hand-laid blocks use depth 1 on 16x16 only"
        return (8, 8)
    cur, prev = mi[y // 4, x // 4], (mi[y // 4, x // 4 - 1] if vert else mi[y // 4 - 1, x // 4])
    c, p = tx(cur)[0 if vert else 1], tx(prev)[0 if vert else 1]
    if (x if vert else y) % c:
        return 0
    m = min(c, p)
    return 4 if m == 4 else 8 if m == 8 else 14
