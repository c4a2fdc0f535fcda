// interintra_plan.h — the rules of inter-intra prediction (interintra.hip), each stated once: the seven block sizes, the
// four modes, build_intra_predictors' edge preparation for them, the DC variant and value, the SMOOTH value and its
// weights, the smooth inter-intra masks, the wedge mask of a plane, the blend, the edge pool's layout and the validation of a
// block.  No HIP runtime: plain C++17 builds it too (tests/interintra_plan_check.cpp); under hipcc what the kernel also
// calls is __host__ __device__.
//
// A block of luma size w x h; plane subsampling ss (0 luma, 1 chroma); the plane's block is pw x ph = (w >> ss) x (h >> ss),
// one of ten sizes from 4x4 to 32x32, so one tile of pred_plan.h.  n_top / n_left are n_top_px / n_left_px of
// build_intra_predictors (EbEncIntraPrediction.c:60-239): how many raw neighbour samples exist above / left of the plane's block.
#pragma once
#include "pred_plan.h"
#include "wedge_masks.h"

namespace interintra_plan {

using pred_plan::log2_of;

enum Mode { kDcPred = 0, kVPred = 1, kHPred = 2, kSmoothPred = 3, kModes = 4 }; // InterIntraMode; interintra_to_intra_mode
enum DcVariant { kDc128 = 0, kDcTop = 1, kDcLeft = 2, kDcBoth = 3 };            // svt_aom_dc_pred[n_left > 0][n_top > 0]

// svt_aom_is_interintra_allowed_bsize: BLOCK_8X8 .. BLOCK_32X32 in enum order, which has no 4:1 shape
constexpr int kSizes[7][2] = {{8, 8}, {8, 16}, {16, 8}, {16, 16}, {16, 32}, {32, 16}, {32, 32}};
PRED_HD bool size_allowed(int wl, int hl) { return wl >= 3 && wl <= 5 && hl >= 3 && hl <= 5 && wl - hl <= 1 && hl - wl <= 1; }
// the ten sizes of a plane's block: the seven, and the chroma of the three smallest
inline bool plane_size_ok(int w, int h) {
    const int wl = log2_of(w), hl = log2_of(h);
    return (1 << wl) == w && (1 << hl) == h && wl >= 2 && wl <= 5 && hl >= 2 && hl <= 5 && wl - hl <= 1 && hl - wl <= 1;
}

// sm_weight_arrays (EbIntraPrediction.c:26-45) for block dimensions 4 .. 32: the weights of dimension d are
// kSmWeights[d - 4 .. 2 d - 4); scale 256
static constexpr __attribute__((aligned(4))) uint8_t kSmWeights[60] = {
    255, 149, 85,  64,  255, 197, 146, 105, 73,  50,  37,  32,  255, 225, 196, 170, 145, 123, 102, 84,
    68,  54,  43,  33,  26,  20,  17,  16,  255, 240, 225, 210, 196, 182, 169, 157, 145, 133, 122, 111,
    101, 92,  83,  74,  66,  59,  52,  45,  39,  34,  29,  25,  21,  17,  14,  12,  10,  9,   8,   8};
// ii_weights1d (EbInterPrediction.c:2137-2145)
static constexpr __attribute__((aligned(16))) uint8_t kIiWeights[128] = {
    60, 58, 56, 54, 52, 50, 48, 47, 45, 44, 42, 41, 39, 38, 37, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 22, 21, 20,
    19, 19, 18, 18, 17, 16, 16, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10, 9,  9,  9,  8,  8,  8,  8,  7,  7,  7,  7,
    6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  4,  4,  4,  4,  4,  4,  4,  4,  3,  3,  3,  3,  3,  3,  3,  3,  3,  2,  2,  2,  2,  2,
    2,  2,  2,  2,  2,  2,  2,  2,  2,  2,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1};
// ii_size_scales[plane_bsize] (:2146-2150): 128 / the plane block's larger side, as a shift
PRED_HD int ii_scale_log2(int pwl, int phl) { return 7 - (pwl > phl ? pwl : phl); }

// AOM_BLEND_A64 (aom_dsp/blend.h): m of a, 64 - m of b; AOM_BLEND_AVG
PRED_HD int blend_a64(int m, int a, int b) { return (m * a + (64 - m) * b + 32) >> 6; }
PRED_HD int blend_avg(int a, int b) { return (a + b + 1) >> 1; }

// ---- the edge preparation of build_intra_predictors / _high for DC, V, H and SMOOTH ----
PRED_HD int base_value(int bd) { return 128 << (bd - 8); }
// Entry i of the prepared above row: the n_top raw samples, the last one repeated; with none the left column's first raw
// sample, or base - 1 when there is no left either.  For V_PRED with n_top == 0 the reference returns early with the whole
// block filled by left[0] or base - 1 (:110-121): the same value as every entry here, so the V predictor on the prepared row is
// that fill.  raw_above / raw_left: the raw neighbour samples of the plane's block (any integer type).
template <typename T> PRED_HD int prepared_above(const T *raw_above, const T *raw_left, int n_top, int n_left, int bd, int i) {
    if (n_top > 0) return raw_above[i < n_top ? i : n_top - 1];
    return n_left > 0 ? (int)raw_left[0] : base_value(bd) - 1;
}
// Entry i of the prepared left column: likewise, with above[0] or base + 1; H_PRED with n_left == 0 is the early fill.
template <typename T> PRED_HD int prepared_left(const T *raw_above, const T *raw_left, int n_top, int n_left, int bd, int i) {
    if (n_left > 0) return raw_left[i < n_left ? i : n_left - 1];
    return n_top > 0 ? (int)raw_above[0] : base_value(bd) + 1;
}
// the early return of :110-121 (need_above is false for H, need_left for V; DC and SMOOTH need both)
PRED_HD bool constant_fill(int mode, int n_top, int n_left) { return (mode == kVPred && n_top == 0) || (mode == kHPred && n_left == 0); }

// ---- the predictors (EbIntraPrediction.c:1041-1134; the highbd forms are the same arithmetic) ----
PRED_HD int dc_variant(int n_top, int n_left) { return (n_left > 0 ? 2 : 0) | (n_top > 0 ? 1 : 0); }
// (sum + (count >> 1)) / count for count = 2^wl + 2^hl of an allowed plane size (equal sides, or 2:1): a shift, or a shift and
// a division by 3 as a multiplication (exact for the quotient's range: tests/interintra_plan_check.cpp holds it to "/")
PRED_HD int dc_divide(int sum, int wl, int hl) {
    const int lo = wl < hl ? wl : hl, v = sum + (((1 << wl) + (1 << hl)) >> 1);
    return wl == hl ? v >> (lo + 1) : (int)(((uint32_t)(v >> lo) * 0xAAABu) >> 17);
}
// the value of every sample of a DC block: sums over the prepared above row (pw entries) and left column (ph entries)
PRED_HD int dc_value(int variant, int sum_above, int sum_left, int pwl, int phl, int bd) {
    if (variant == kDcBoth) return dc_divide(sum_above + sum_left, pwl, phl);
    if (variant == kDcTop) return (sum_above + ((1 << pwl) >> 1)) >> pwl;
    if (variant == kDcLeft) return (sum_left + ((1 << phl) >> 1)) >> phl;
    return base_value(bd);
}
// smooth_predictor at (r, c): above_c = above[c], left_r = left[r], below = left[ph - 1], right = above[pw - 1]; divide_round by 9
PRED_HD int smooth_value(int above_c, int left_r, int below, int right, int pw, int ph, int r, int c) {
    const int wh = kSmWeights[ph - 4 + r], ww = kSmWeights[pw - 4 + c];
    return (wh * above_c + (256 - wh) * below + ww * left_r + (256 - ww) * right + 256) >> 9;
}

// ---- the masks ----
// build_smooth_interintra_mask (EbInterPrediction.c:2153-2188) at (r, c) of the plane's block
PRED_HD int smooth_mask(int mode, int pwl, int phl, int r, int c) {
    if (mode == kDcPred) return 32;
    const int k = mode == kVPred ? r : mode == kHPred ? c : (r < c ? r : c);
    return kIiWeights[k << ii_scale_log2(pwl, phl)];
}
// the wedge mask a plane's blend reads: that of the LUMA size (wl, hl), sign INTERINTRA_WEDGE_SIGN = 0; for chroma
// svt_aom_blend_a64_mask's subw = subh = 1 form: ROUND_POWER_OF_TWO of the 2x2 sum by 2
PRED_HD int wedge_mask_plane(const wedge_masks::Plan &p, int ss, int r, int c) {
    if (!ss) return wedge_masks::plan_value(p, r, c);
    return (wedge_masks::plan_value(p, 2 * r, 2 * c) + wedge_masks::plan_value(p, 2 * r + 1, 2 * c) +
            wedge_masks::plan_value(p, 2 * r, 2 * c + 1) + wedge_masks::plan_value(p, 2 * r + 1, 2 * c + 1) + 2) >> 2;
}

// ---- the edge pool: per block above[w], left[h] of luma, then above[w / 2], left[h / 2] of Cb and of Cr ----
PRED_HD int edge_plane_offset(int wl, int hl, int plane) {
    const int n = (1 << wl) + (1 << hl);
    return plane == 0 ? 0 : plane == 1 ? n : n + (n >> 1);
}
PRED_HD int edge_samples(int wl, int hl, int nplanes) { return ((1 << wl) + (1 << hl)) * (nplanes > 1 ? 2 : 1); }

// ---- a block: everything but the picture rectangle (pred_plan::check_block_rect) and the reference index ----
inline bool reserved_ok(const SvtGpuInterIntraBlock &b) {
    for (uint8_t v : b.reserved)
        if (v) return false;
    return true;
}
inline bool counts_ok(const SvtGpuInterIntraBlock &b, int nplanes) {
    for (int q = 0; q < (nplanes > 1 ? 2 : 1); q++)
        if (b.n_top[q] > ((1 << b.w_log2) >> q) || b.n_left[q] > ((1 << b.h_log2) >> q)) return false;
    return true;
}
inline bool edges_ok(const SvtGpuInterIntraBlock &b, int nplanes, int64_t n_edges) {
    return b.edge_offset >= 0 && (int64_t)b.edge_offset + edge_samples(b.w_log2, b.h_log2, nplanes) <= n_edges;
}
// with_mode: the predict entry; the mode-SSE entry does not look at mode, use_wedge and wedge_index
inline bool block_ok(const SvtGpuInterIntraBlock &b, int nplanes, int64_t n_edges, bool with_mode) {
    if (!size_allowed(b.w_log2, b.h_log2) || b.filter_x > 3 || b.filter_y > 3 || !reserved_ok(b)) return false;
    if (with_mode && (b.mode > 3 || b.use_wedge > 1 || b.wedge_index > 15)) return false;
    return counts_ok(b, nplanes) && edges_ok(b, nplanes, n_edges);
}

} // namespace interintra_plan
