// compound_tile.h — the tile machinery shared by the two-reference predictors: compound.hip (COMPOUND_AVERAGE,
// COMPOUND_DISTWTD) and masked_compound.hip (COMPOUND_WEDGE, COMPOUND_DIFFWTD).  Both run the same two reference passes
// per tile and differ only in how the two CONV_BUF_TYPE values of a sample become a pixel.
//
//   unit         four horizontally adjacent outputs of a tile: what one lane computes at a time.  A tile of tw x th outputs
//                (at most 32 x 32) has tw * th / 4 units; unit u is row u / (tw / 4), columns 4 * (u % (tw / 4)) .. + 3.
//   tile pass    one reference of one tile: the lanes stage rows -3 .. th + 3 and columns -4 .. tw + 3 of the reference
//                (every coordinate clamped into the readable border; groups of four columns, one load where no clamp
//                acts) into the tile's LDS window as 16-bit samples, whose row stride tw + 8 keeps every group of four
//                8-byte aligned.  The 2-D form then runs the horizontal filter into an int16 LDS intermediate of th + 7
//                rows; the last step of every form (x, y, copy: from the window; 2-D: from the intermediate) gives a
//                unit's four CONV_BUF_TYPE values from 8-byte LDS reads.  Each form restates its own C function.
//   wave item    what one wave does: one tile of 64 or more units, or 64 / units tiles of one shape side by side, lane
//                l on tile l / units ("slot").  So four 8x8 luma blocks, or the sixteen 4x4 chroma blocks of eight 8x8
//                blocks, fill a wave.  The host builds the item list while it checks the blocks.
//
// LDS: slot s of a wave uses window [s * (th + 7) * (tw + 8), + (th + 7) * (tw + 8)) and intermediate
// [s * (th + 7) * tw, + (th + 7) * tw); the largest are one 32x32 tile (39 * 40 = 1560, 39 * 32 = 1248) and sixteen 4x4
// tiles (16 * 132 = 2112, 16 * 44 = 704) <= kWinCap, kImCap.
#pragma once
#include <cstring>
#include <vector>

#include "conv_device.h"
#include "interp_tables.h"
#include "svtgpu_internal.h"

namespace compound_tile {

using namespace conv_device;

constexpr int kMaxRefs = 26; // as svtgpu_tf_predict_frame
constexpr int kTile    = 32;
constexpr int kWinCap  = 2112, kImCap = 1248, kWaveLds = kWinCap + kImCap; // 16-bit elements per wave
constexpr int kMaxSlots = 16;
enum { kCopy = 0, kHorz = 1, kVert = 2, k2d = 3 };

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef int16_t  i16x4 __attribute__((ext_vector_type(4)));
typedef int16_t  i16x8 __attribute__((ext_vector_type(8)));
typedef uint8_t  u8x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Vec4;
template <> struct Vec4<uint8_t> { typedef u8x4 type; };
template <> struct Vec4<uint16_t> { typedef u16x4 type; };

struct Rounds {
    int32_t r0, r1, bd;
};

__device__ __forceinline__ void load_taps(const int16_t *p, int f[8]) { // a 16-byte aligned row of eight taps
    const i16x8 v = *(const i16x8 *)p;
#pragma unroll
    for (int k = 0; k < 8; k++) f[k] = v[k];
}

// One lane's part of staging a tile's window.  ref points at sample (0, 0) of a plane readable over [x_lo, x_hi] x
// [y_lo, y_hi]; window row r, column c holds the sample at (sx - 4 + c, sy - 3 + r).  Rows 3 .. th + 2 only when the form
// has no vertical filter.
template <typename T>
__device__ __forceinline__ void stage_window(const T *__restrict__ ref, int stride, int x_lo, int x_hi, int y_lo, int y_hi,
                                             int sx, int sy, int tw, int th, int mode, uint16_t *win, int li, int lps) {
    const int ws = tw + 8, g = ws >> 2; // g in {3, 4, 6, 10}
    const int r_first = (mode & kVert) ? 0 : 3, r_cnt = (mode & kVert) ? th + 7 : th;
    const int recip = (1 << 20) / g + 1; // u / g, exact for u < 39 * 10 (the error is below u / 2^20 < 1 / g)
    for (int u = li; u < r_cnt * g; u += lps) {
        const int rr = (u * recip) >> 20, cg = u - rr * g, row = r_first + rr;
        const int gy = clamp_i(sy - 3 + row, y_lo, y_hi), gx = sx - 4 + 4 * cg;
        const T  *p = ref + (ptrdiff_t)gy * stride;
        u16x4     v;
        if (gx >= x_lo && gx + 3 <= x_hi) {
            T t[4];
            __builtin_memcpy(t, p + gx, sizeof t);
            v = (u16x4){t[0], t[1], t[2], t[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = p[clamp_i(gx + k, x_lo, x_hi)];
        }
        *(u16x4 *)(win + row * ws + 4 * cg) = v;
    }
}

// The 2-D form's horizontal pass (svt_av1_jnt_convolve_2d_c :516-527): window rows 0 .. th + 6 into im[th + 7][tw].
__device__ __forceinline__ void horizontal_to_im(const uint16_t *win, int16_t *im, int twl, int th, const int fx[8], Rounds cr,
                                                 int li, int lps) {
    const int tw = 1 << twl, ws = tw + 8, gl = twl - 2;
    for (int u = li; u < (th + 7) << gl; u += lps) {
        const int    rr = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
        const u16x4 *p = (const u16x4 *)(win + rr * ws + x4);
        const u16x4  a = p[0], b = p[1], c = p[2];
        const int    s[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
        i16x4        o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int sum = 1 << (cr.bd + 6);
#pragma unroll
            for (int k = 0; k < 8; k++) sum += fx[k] * s[j + 1 + k];
            o[j] = (int16_t)round_shift(sum, cr.r0);
        }
        *(i16x4 *)(im + rr * tw + x4) = o;
    }
}

// The four CONV_BUF_TYPE values of the unit at row y, columns x4 .. x4 + 3, by the form's own C function: copy
// (:641-677), x (:599-639), y (:557-597), 2-D's vertical pass (:529-554).  The 2-D and copy forms hold the value in a
// uint16_t, the x and y forms in an int32_t.
__device__ __forceinline__ void final_unit(int mode, const uint16_t *win, const int16_t *im, int tw, int y, int x4,
                                           const int fx[8], const int fy[8], Rounds cr, int res[4]) {
    const int ws = tw + 8, offset_bits = cr.bd + 14 - cr.r0;
    const int round_offset = (1 << (offset_bits - cr.r1)) + (1 << (offset_bits - cr.r1 - 1));
    if (mode == kCopy) {
        const u16x4 v = *(const u16x4 *)(win + (y + 3) * ws + x4 + 4);
        const int   bits = 14 - cr.r0 - cr.r1;
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = (uint16_t)((uint16_t)((int)v[j] << bits) + (uint16_t)round_offset);
    } else if (mode == kHorz) {
        const u16x4 *p = (const u16x4 *)(win + (y + 3) * ws + x4);
        const u16x4  a = p[0], b = p[1], c = p[2];
        const int    s[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) sum += fx[k] * s[j + 1 + k];
            res[j] = (1 << (7 - cr.r1)) * round_shift(sum, cr.r0) + round_offset;
        }
    } else if (mode == kVert) {
        int sum[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u16x4 v = *(const u16x4 *)(win + (y + k) * ws + x4 + 4);
#pragma unroll
            for (int j = 0; j < 4; j++) sum[j] += fy[k] * (int)v[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = round_shift(sum[j] * (1 << (7 - cr.r0)), cr.r1) + round_offset;
    } else {
        int sum[4] = {1 << offset_bits, 1 << offset_bits, 1 << offset_bits, 1 << offset_bits};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const i16x4 v = *(const i16x4 *)(im + (y + k) * tw + x4);
#pragma unroll
            for (int j = 0; j < 4; j++) sum[j] += fy[k] * (int)v[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = (uint16_t)round_shift(sum[j], cr.r1);
    }
}

// One reference pass of a tile for one lane: stage, (2-D: horizontal pass,) then emit(i, y, x4, res) for the lane's units
// u = li + i * lps < units, i < 4.  Every lane of the wave that is in a slot calls it; the lanes of a slot share win / im.
template <typename T, typename Emit>
__device__ __forceinline__ void tile_pass(const T *__restrict__ ref, int stride, int x_lo, int x_hi, int y_lo, int y_hi, int sx,
                                          int sy, int twl, int thl, int mode, const int16_t *fxp, const int16_t *fyp, Rounds cr,
                                          uint16_t *win, int16_t *im, int li, int lps, Emit emit) {
    const int tw = 1 << twl, th = 1 << thl, gl = twl - 2, units = 1 << (twl + thl - 2);
    int       fx[8], fy[8];
    load_taps(fxp, fx);
    load_taps(fyp, fy);
    stage_window<T>(ref, stride, x_lo, x_hi, y_lo, y_hi, sx, sy, tw, th, mode, win, li, lps);
    wave_lds_sync();
    if (mode == k2d) horizontal_to_im(win, im, twl, th, fx, cr, li, lps);
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = li + i * lps;
        if (u < units) {
            const int y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
            int       res[4];
            final_unit(mode, win, im, tw, y, x4, fx, fy, cr, res);
            emit(i, y, x4, res);
        }
    }
    wave_lds_sync(); // this pass's LDS reads before the next pass's stores
}

struct CompSlot { // one tile: block, plane, the tile's origin in the block's plane (samples)
    uint32_t blk;
    uint8_t  plane, ox, oy, reserved;
};
struct CompItem { // one wave's work: nslots tiles of 2^tw_log2 x 2^th_log2 outputs
    CompSlot slot[kMaxSlots];
    uint8_t  tw_log2, th_log2, nslots, reserved[13];
};
static_assert(sizeof(CompItem) == 144 && sizeof(CompItem) % 16 == 0, "CompItem is 144 bytes");

// av1_get_interp_filter_params_with_block_size: the table of filter kind `kind` for a dimension of `size` samples
__device__ __forceinline__ int filter_table(int kind, int size) {
    if (size <= 4 && (kind == kInterpRegular || kind == kInterpSharp)) return kInterpRegular4;
    if (size <= 4 && kind == kInterpSmooth) return kInterpSmooth4;
    return kind;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline bool   size_ok(int v) { return v >= 4 && v <= 128 && !(v & (v - 1)); }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the AV1 block sizes a compound may have (is_comp_ref_allowed: min(w, h) >= 8): 8x8 .. 128x128, ratio at most 4, and
// 128 only beside 64 or 128
inline bool block_size_ok(int wl, int hl) {
    if (wl < 3 || wl > 7 || hl < 3 || hl > 7) return false;
    const int d = wl > hl ? wl - hl : hl - wl;
    return d <= 2 && !((wl == 7 || hl == 7) && d > 1);
}

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

} // namespace compound_tile
