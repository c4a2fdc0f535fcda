// compound_weights.h — the frame-distance weights of AV1's distance-weighted compound (COMPOUND_DISTWTD): the two tables and
// the selection loop of svt_av1_dist_wtd_comp_weight_assign (EbInterPrediction.c:276-318), held to the reference's table walk
// on every (d0, d1, order_idx) of [0, 33]^2 x {0, 1} by tests/test_compound.py.  Plain C++: no HIP in it, a host compiler
// can include it (as csrc/dlf_levels.h and csrc/cdef_pick_plan.h).
#pragma once
#include <cstdint>

namespace compound_weights {

constexpr int kMaxFrameDistance = 31; // MAX_FRAME_DISTANCE; the two offsets sum to 1 << DIST_PRECISION_BITS (pred_plan.h)

constexpr int kQuantDistWeight[4][2]         = {{2, 3}, {2, 5}, {2, 7}, {1, kMaxFrameDistance}};
constexpr int kQuantDistLookupTable[2][4][2] = {
    {{9, 7}, {11, 5}, {12, 4}, {13, 3}},
    {{7, 9}, {5, 11}, {4, 12}, {3, 13}},
};

// d0: |distance from the current frame to the forward reference|, d1: |distance to the backward reference|, both as the
// caller computed them (>= 0; clamped to MAX_FRAME_DISTANCE here, as the reference clamps them); order_idx 0 or 1.
// false: an argument outside that.
inline bool select(int32_t d0, int32_t d1, int32_t order_idx, int32_t *fwd_offset, int32_t *bck_offset) {
    if (d0 < 0 || d1 < 0 || order_idx < 0 || order_idx > 1 || !fwd_offset || !bck_offset) return false;
    d0 = d0 > kMaxFrameDistance ? kMaxFrameDistance : d0;
    d1 = d1 > kMaxFrameDistance ? kMaxFrameDistance : d1;
    const int order = d0 <= d1;
    int       i     = 3;
    if (d0 != 0 && d1 != 0) {
        for (i = 0; i < 3; ++i) {
            const int d0_c0 = d0 * kQuantDistWeight[i][order], d1_c1 = d1 * kQuantDistWeight[i][!order];
            if ((d0 > d1 && d0_c0 < d1_c1) || (d0 <= d1 && d0_c0 > d1_c1)) break;
        }
    }
    *fwd_offset = kQuantDistLookupTable[order_idx][i][order];
    *bck_offset = kQuantDistLookupTable[order_idx][i][1 - order];
    return true;
}

} // namespace compound_weights
