// obmc_plan.h — the rules of OBMC prediction (obmc_pred.hip), each stated once: the 1-D masks, the blend, the geometry of a
// neighbour strip per plane and direction, the filter taps and the MV clamp of a strip, the validation of a block's
// neighbour lists, and the region passes of a tile.  No HIP runtime: plain C++17 builds it too
// (tests/obmc_plan_check.cpp); under hipcc what the kernel also calls is __host__ __device__.
//
// A block of luma size w x h at luma (x, y); plane subsampling ss (0 luma, 1 chroma); direction 0 = above, 1 = left.  A
// neighbour span is (rel, size) in units of 4 luma samples along the shared edge.  "side" is the block's dimension across
// the edge of a direction: h for above, w for left.
#pragma once
#include "pred_plan.h"

namespace obmc_plan {

using pred_plan::log2_of;

// obmc_mask_1/2/4/8/16/32 (EbInterPrediction.c:2416-2426): the mask of length L is kMasks[L .. 2L)
static constexpr __attribute__((aligned(16))) uint8_t kMasks[64] = {
    0,  64, 45, 64, 39, 50, 59, 64, 36, 42, 48, 53, 57, 61, 64, 64, 34, 37, 40, 43, 46, 49, 52, 54, 56, 58, 60, 61, 64, 64, 64, 64,
    33, 35, 36, 38, 40, 41, 43, 44, 45, 47, 48, 50, 51, 52, 53, 55, 56, 57, 58, 59, 60, 60, 61, 62, 64, 64, 64, 64, 64, 64, 64, 64};
// svt_av1_get_obmc_mask (:2428-2438); nullptr for a length it has no mask for
inline const uint8_t *mask_of(int length) {
    return (length == 1 || length == 2 || length == 4 || length == 8 || length == 16 || length == 32) ? kMasks + length : nullptr;
}
// AOM_BLEND_A64 (aom_dsp/blend.h): m of a, 64 - m of b
PRED_HD int blend_a64(int m, int a, int b) { return (m * a + (64 - m) * b + 32) >> 6; }

// max_neighbor_obmc (EbEncInterPrediction.c:679) by the log2 of the side in units of 4
constexpr int kMaxNeighbours[6] = {0, 1, 2, 3, 4, 4};
inline int    max_neighbours(int side) { return kMaxNeighbours[log2_of(side >> 2)]; }

// build_prediction_by_{above,left}_pred (:1176-1178, :1276-1278): the depth across the edge that the reference predicts
PRED_HD int pred_depth(int side, int ss) {
    const int v = side >> (ss + 1), hi = 64 >> (ss + 1);
    return v < 4 ? 4 : v > hi ? hi : v;
}
// build_obmc_inter_pred_{above,left} (:1448-1456, :1495-1502): the depth that is blended, which is the mask's length
PRED_HD int blend_depth(int side, int ss) { return ((side < 64 ? side : 64) >> 1) >> ss; }
// svt_av1_skip_u4x4_pred_in_obmc (EbInterPrediction.c:2291-2307) with DISABLE_CHROMA_U8X8_OBMC == 0: a plane block of 4x4,
// 8x4 or 4x8 takes no above strip
PRED_HD bool skip_plane(int w, int h, int ss, int dir) {
    const int pw = w >> ss, ph = h >> ss;
    return dir == 0 && ((pw == 4 && (ph == 4 || ph == 8)) || (pw == 8 && ph == 4));
}

// clamp_mv_to_umv_border_sb (EbEncInterPrediction.c:28-48) with the edges and the spel size given separately: the region
// starts at luma `org` and is `extent` luma samples long in a picture of `dim`; spel_size is the predicted size in the plane.
// pred_plan::clamped_mv(mv, org, b, dim, ss) is clamped_mv_ex(mv, org, b, b >> ss, dim, ss).
PRED_HD int clamped_mv_ex(int mv, int org, int extent, int spel_size, int dim, int ss) {
    const int sc = 1 - ss, q = (int16_t)(mv * (1 << sc)), spel = (4 + spel_size) << 4;
    const int lo = -(org * 8) * (1 << sc) - spel, hi = ((dim - extent - org) * 8) * (1 << sc) + spel - 16;
    return (int16_t)(q < lo ? lo : q > hi ? hi : q);
}
// A strip's MV component along the shared edge (av1_setup_build_prediction_by_{above,left}_pred, :754-788): the edges are
// the span's.  org the block's luma origin in that direction.
PRED_HD int strip_mv_along(int mv, int org, int rel, int size, int dim, int ss) {
    return clamped_mv_ex(mv, org + 4 * rel, 4 * size, (4 * size) >> ss, dim, ss);
}
// ... and across it (build_prediction_by_{above,left}_preds, :1353-1355, :1395-1397): the block's origin with an extent of
// min(side / 2, 32) luma; the spel size is the predicted depth, which is 4 where extent >> 1 is 2 (chroma of a side of 8)
PRED_HD int strip_mv_across(int mv, int org, int side, int dim, int ss) {
    const int e = side / 2 < 32 ? side / 2 : 32;
    return clamped_mv_ex(mv, org, e, pred_depth(side, ss), dim, ss);
}
// av1_get_convolve_filter_params on the strip's predicted dimensions: the size in the plane that chooses 4 or 8 taps
PRED_HD int strip_size_along(int size, int ss) { return (4 * size) >> ss; }

// One list of a block: sizes powers of two from 2 to 16, rel even, spans ascending without overlap inside the side, at most
// max_neighbor_obmc of them, none where the picture has no neighbour (org == 0).  `side_along` is the block's dimension
// along the shared edge (w for the above list).
inline bool list_ok(const SvtGpuObmcNeighbour *nb, int n, int side_along, int org_across) {
    if (n < 0 || n > max_neighbours(side_along) || (n && org_across == 0)) return false;
    int end = 0;
    for (int k = 0; k < n; k++) {
        const int s = nb[k].size;
        if (s < 2 || s > 16 || (s & (s - 1)) || (nb[k].rel & 1) || nb[k].rel < end || nb[k].rel + s > side_along / 4) return false;
        end = nb[k].rel + s;
    }
    return true;
}
inline bool lists_ok(const SvtGpuObmcBlock &b) {
    return b.n_above <= 4 && b.n_left <= 4 && list_ok(b.nb, b.n_above, 1 << b.w_log2, b.y) &&
           list_ok(b.nb + 4, b.n_left, 1 << b.h_log2, b.x);
}
inline bool reserved_ok(const SvtGpuObmcBlock &b) {
    if (b.reserved0) return false;
    for (uint8_t v : b.reserved)
        if (v) return false;
    return true;
}

// The region pass of one span over one tile: the part of the tile (plane samples [ox, ox + tw) x [oy, oy + th) of the
// block's plane) that the span's strip blends, as a rectangle relative to the tile.  Its width is a multiple of 4 (a lane
// computes four adjacent samples): a left strip two columns deep (chroma of a width of 8) is computed four wide, inside the
// four columns the reference predicts, and blended over `depth` columns.  false: the span does not touch the tile.
struct Rect {
    int x0, y0, w, h;
};
PRED_HD bool span_rect(int dir, int w, int h, int ss, int rel, int size, int ox, int oy, int tw, int th, Rect *r, int *depth) {
    if (skip_plane(w, h, ss, dir)) return false;
    const int d = blend_depth(dir ? w : h, ss), a0 = (4 * rel) >> ss, a1 = a0 + ((4 * size) >> ss); // [a0, a1) along the edge
    const int t0 = dir ? oy : ox, tl = dir ? th : tw, c0 = dir ? ox : oy, cl = dir ? tw : th;        // the tile along / across
    if (c0 >= d) return false;
    const int lo = a0 > t0 ? a0 : t0, hi = a1 < t0 + tl ? a1 : t0 + tl;
    if (lo >= hi) return false;
    int across = d - c0 < cl ? d - c0 : cl;
    if (dir && across < 4) across = 4;
    *depth = d;
    if (dir) r->x0 = 0, r->y0 = lo - t0, r->w = across, r->h = hi - lo;
    else r->x0 = lo - t0, r->y0 = 0, r->w = hi - lo, r->h = across;
    return true;
}

} // namespace obmc_plan
