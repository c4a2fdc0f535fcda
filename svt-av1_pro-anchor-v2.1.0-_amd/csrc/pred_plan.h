// pred_plan.h — the host policy of the block predictors (interp.hip, compound.hip, masked_compound.hip, warp.hip), each
// rule stated once: limits, a wave's LDS budget, the wave items and their builders, the batch entries' checks, the MV
// clamp, the metadata layout.  No HIP runtime: plain C++17 builds it too (tests/pred_plan_check.cpp); under hipcc what a
// kernel also calls is __host__ __device__.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/svtgpu.h"

#ifdef __HIPCC__
#define PRED_HD __host__ __device__ __forceinline__
#else
#define PRED_HD inline
#endif

namespace pred_plan {

constexpr int kMaxRefs = 26; // as svtgpu_tf_filter_frame
constexpr int kTile    = 32; // the largest region (interp.hip) or tile (compound_tile.h) of one wave
// 16-bit LDS elements of a wave of the tile kernels.  Slot s of a wave uses window [s * (th + 7) * (tw + 8), + (th + 7) *
// (tw + 8)) and intermediate [s * (th + 7) * tw, + (th + 7) * tw); the largest are one 32x32 tile (39 * 40 = 1560, 39 * 32
// = 1248) and sixteen 4x4 tiles (16 * 132 = 2112, 16 * 44 = 704).  tests/pred_plan_check.cpp holds every item to it.
constexpr int kWinCap = 2112, kImCap = 1248, kWaveLds = kWinCap + kImCap;
constexpr int kMaxSlots = 16;
constexpr int kDistPrecisionBits = 4; // DIST_PRECISION_BITS: COMPOUND_DISTWTD's two offsets sum to 1 << 4

// sizes and rounds
inline bool   size_ok(int v, int min_size) { return v >= min_size && v <= 128 && !(v & (v - 1)); } // the shims' w and h
inline bool   rounds_ok(int r0, int r1) { return r0 >= 0 && r0 <= 7 && r1 >= 0 && r1 <= 7 && 14 - r0 - r1 >= 0; }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline int    log2_of(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}

// the AV1 block sizes a compound may have (is_comp_ref_allowed: min(w, h) >= 8): 8x8 .. 128x128, ratio at most 4, and
// 128 only beside 64 or 128
inline bool block_size_ok(int wl, int hl) {
    if (wl < 3 || wl > 7 || hl < 3 || hl > 7) return false;
    const int d = wl > hl ? wl - hl : hl - wl;
    return d <= 2 && !((wl == 7 || hl == 7) && d > 1);
}

// the arguments every batch entry takes (after n_refs > kMaxRefs, which is SVTGPU_ERR_UNSUPPORTED); warp has no border
inline bool batch_args_ok(const void *state, const void *refs, int n_refs, const void *blocks, int n_blocks, int bit_depth,
                          const void *pred, int border_x = 0, int border_y = 0) {
    return state && refs && pred && n_refs >= 0 && n_blocks >= 0 && (!n_blocks || blocks) &&
           (bit_depth == 8 || bit_depth == 10) && border_x >= 0 && border_y >= 0;
}
// every reference's planes: present, sample-aligned, a row as wide as the picture and its declared border on both sides
inline bool ref_planes_ok(const SvtGpuTfPlanes *refs, int n_refs, int width, int border_x, int bit_depth, int nplanes) {
    const int bs = bit_depth > 8 ? 2 : 1;
    for (int r = 0; r < n_refs; r++)
        for (int p = 0; p < nplanes; p++) {
            const int ss = p > 0;
            if (!refs[r].plane[p] || ((uintptr_t)refs[r].plane[p] & (bs - 1)) ||
                refs[r].stride[p] < (width >> ss) + 2 * (border_x >> ss))
                return false;
        }
    return true;
}
// a predictor's planes: present, 16-byte aligned rows (the kernels store vectors) of at least `width` luma samples
inline bool pred_planes_ok(const SvtGpuTfPlanes &pred, int width, int bit_depth, int nplanes) {
    const int bs = bit_depth > 8 ? 2 : 1;
    for (int p = 0; p < nplanes; p++)
        if (!pred.plane[p] || pred.stride[p] < (width >> (p > 0)) || (((size_t)pred.stride[p] * bs) & 15) ||
            ((uintptr_t)pred.plane[p] & 15))
            return false;
    return true;
}
// both, for a picture of `width` luma samples (no check involves its height); without chroma (nplanes = 1) planes 1 and
// 2 are not looked at
inline bool check_planes(const SvtGpuTfPlanes *refs, int n_refs, const SvtGpuTfPlanes *pred, int width, int border_x,
                         int bit_depth, int nplanes) {
    return ref_planes_ok(refs, n_refs, width, border_x, bit_depth, nplanes) && pred_planes_ok(*pred, width, bit_depth, nplanes);
}
// a block of an allowed size at a non-negative origin that is a multiple of `align`, inside width x height
inline bool check_block_rect(int x, int y, int wl, int hl, int align, int width, int height) {
    return block_size_ok(wl, hl) && x >= 0 && y >= 0 && !(x & (align - 1)) && !(y & (align - 1)) && x + (1 << wl) <= width &&
           y + (1 << hl) <= height;
}
inline bool dist_wtd_ok(int dist_wtd, int fwd, int bck) {
    return dist_wtd <= 1 && (!dist_wtd || fwd + bck == (1 << kDistPrecisionBits));
}
// One component of clamp_mv_to_umv_border_sb (EbEncInterPrediction.c:28-48) with the block's own edges: mv in 1/8 luma
// sample of a block of luma size b at luma origin org in a picture of luma size dim -> the MV in 1/16 sample of the plane
// (ss = 1: chroma), cast to int16 before and after the clamp as the reference's MV struct does.  Phase = & 15, integer
// part = >> 4 (arithmetic).
PRED_HD int clamped_mv(int mv, int org, int b, int dim, int ss) {
    const int sc = 1 - ss, q = (int16_t)(mv * (1 << sc)), spel = (4 + (b >> ss)) << 4;
    const int lo = -(org * 8) * (1 << sc) - spel, hi = ((dim - b - org) * 8) * (1 << sc) + spel - 16;
    return (int16_t)(q < lo ? lo : q > hi ? hi : q);
}

// the tile kernels' wave items (compound_tile.h says what a unit, a tile pass and a slot are)
struct CompSlot { // one tile: block, plane, the tile's origin in the block's plane (samples)
    uint32_t blk;
    uint8_t  plane, ox, oy, reserved;
};
struct CompItem { // one wave's work: nslots tiles of 2^tw_log2 x 2^th_log2 outputs
    CompSlot slot[kMaxSlots];
    uint8_t  tw_log2, th_log2, nslots, reserved[13];
};
static_assert(sizeof(CompItem) == 144 && sizeof(CompItem) % 16 == 0, "CompItem is 144 bytes");

struct ItemBuilder { // tiles -> wave items; small tiles of one shape gathered, up to 64 / units to an item
    std::vector<CompItem> items;
    int                   open[3][3]; // the item still taking slots for tile shape (tw_log2 - 2, th_log2 - 2), or -1
    ItemBuilder() {
        for (auto &row : open)
            for (int &v : row) v = -1;
    }
    void add(uint32_t blk, int plane, int ox, int oy, int twl, int thl) {
        const int units = 1 << (twl + thl - 2), cap = units >= 64 ? 1 : 64 / units;
        int      *slot_of = cap > 1 && twl <= 4 && thl <= 4 ? &open[twl - 2][thl - 2] : nullptr; // cap > 1 only for shapes up to 16x4 / 8x8 / 4x16
        int       k = slot_of ? *slot_of : -1;
        if (k < 0) {
            CompItem it;
            memset(&it, 0, sizeof it);
            it.tw_log2 = (uint8_t)twl, it.th_log2 = (uint8_t)thl;
            items.push_back(it);
            k = (int)items.size() - 1;
        }
        CompItem &it = items[k];
        CompSlot &s  = it.slot[it.nslots++];
        s.blk = blk, s.plane = (uint8_t)plane, s.ox = (uint8_t)ox, s.oy = (uint8_t)oy;
        if (slot_of) *slot_of = it.nslots < cap ? k : -1;
    }
    // every tile (at most 32 x 32) of plane `plane` of a block of luma size 2^wl x 2^hl
    void add_plane(uint32_t blk, int plane, int wl, int hl) {
        const int pwl = wl - (plane > 0), phl = hl - (plane > 0), twl = pwl < 5 ? pwl : 5, thl = phl < 5 ? phl : 5;
        for (int oy = 0; oy < (1 << phl); oy += 1 << thl)
            for (int ox = 0; ox < (1 << pwl); ox += 1 << twl) add(blk, plane, ox, oy, twl, thl);
    }
};

// the warp kernel's items (warp.hip says what a unit is)
struct WarpItem { // one workgroup: n units of one plane of one block, wave v on unit (ux + v % gw, uy + v / gw)
    uint32_t blk;
    uint8_t  plane, ux, uy, shape; // warp_shape_encode(gw, n)
};
PRED_HD uint8_t warp_shape_encode(int gw, int n) { return (uint8_t)((gw - 1) | (n << 4)); } // gw 1 or 2, n 1 .. 4
PRED_HD void    warp_shape_decode(uint8_t shape, int *gw, int *n) { *gw = (shape & 1) + 1, *n = shape >> 4; }

// The items of block `blk` of luma size 2^wl x 2^hl: up to 2 x 2 units of a plane to an item (1 x 4 for a plane 8 wide).
// Chroma is warped for blocks of at least 16 x 16 (EbEncInterPrediction.c:2849); smaller ones get luma only.
// emit(item) per item: the caller appends, so the loop is part of the caller's own per-block loop.
template <typename Emit> inline void warp_items(uint32_t blk, int wl, int hl, bool chroma, Emit emit) {
    const int np = (chroma && wl >= 4 && hl >= 4) ? 3 : 1;
    for (int p = 0; p < np; p++) {
        const int uw = ((1 << wl) >> (p > 0)) >> 3, uh = ((1 << hl) >> (p > 0)) >> 3, gw = uw >= 2 ? 2 : 1, gh = 4 / gw;
        for (int uy = 0; uy < uh; uy += gh)
            for (int ux = 0; ux < uw; ux += gw) {
                const int rows = uh - uy < gh ? uh - uy : gh;
                emit(WarpItem{blk, (uint8_t)p, (uint8_t)ux, (uint8_t)uy, warp_shape_encode(gw, rows * gw)});
            }
    }
}

// a batch call's metadata buffer: the reference descriptors, the blocks as the kernel reads them, the items
struct MetaLayout {
    size_t ref_bytes, blk_bytes, item_bytes, o_blk, o_item, total; // the references are at 0
    MetaLayout(size_t n_refs, size_t n_blocks, size_t block_size, size_t n_items, size_t item_size)
        : ref_bytes(n_refs * sizeof(SvtGpuTfPlanes)), blk_bytes(n_blocks * block_size), item_bytes(n_items * item_size),
          o_blk(align16(ref_bytes)), o_item(o_blk + align16(blk_bytes)), total(o_item + item_bytes) {} // both offsets 16-aligned
};

} // namespace pred_plan
