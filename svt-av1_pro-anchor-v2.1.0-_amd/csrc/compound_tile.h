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
//                blocks, fill a wave.  The host builds the item list while it checks the blocks (pred_plan::ItemBuilder).
//
// The constants, the items (CompItem, ItemBuilder) and the LDS budget of a wave are pred_plan.h's; here is what runs on
// the device with them, and the upload of a batch call's metadata.
#pragma once
#include "conv_device.h"
#include "interp_tables.h"
#include "svtgpu_internal.h"

namespace compound_tile {

using namespace conv_device;
using namespace pred_plan;

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
    const int ws = tw + 8, g = ws >> 2; // g in {3, 4, 6, 10} for a tile; 3 .. 10 for obmc_pred.hip's rectangles (tw a multiple of 4 up to 32)
    const int r_first = (mode & kVert) ? 0 : 3, r_cnt = (mode & kVert) ? th + 7 : th;
    const int recip = (1 << 20) / g + 1; // u / g, exact for u < 39 * 10 and every g up to 10 (the error is below u / 2^20 < 1 / g)
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

// av1_get_interp_filter_params_with_block_size: the table of filter kind `kind` for a dimension of `size` samples
__device__ __forceinline__ int filter_table(int kind, int size) {
    if (size <= 4 && (kind == kInterpRegular || kind == kInterpSharp)) return kInterpRegular4;
    if (size <= 4 && kind == kInterpSmooth) return kInterpSmooth4;
    return kind;
}

// One reference (r = 0 or 1) of a tile for one lane, from what both tile kernels hold after their preamble: the block b, the
// tile's slot sl, the block's origin (px, py) in the slot's plane; `a` the kernel's arguments; emit as tile_pass.  The
// preamble stays in each kernel: behind a shared function the masked kernel's registers change (profiles/pred_plan_refactor).
template <typename T, typename Args, typename Block, typename Emit>
__device__ __forceinline__ void ref_pass(const Args &a, const Block &b, const CompSlot &sl, int r, int px, int py, int twl, int thl,
                                         Rounds cr, uint16_t *win, int16_t *im, int li, int lps, Emit emit) {
    const int p = sl.plane, ss = p > 0;
    const SvtGpuTfPlanes &rp = a.refs[r ? b.ref1 : b.ref0];
    const int bw = 1 << b.w_log2, bh = 1 << b.h_log2, pbw = bw >> ss, pbh = bh >> ss; // the block in luma and in the plane
    const int pw = a.width >> ss, ph = a.height >> ss, bdx = a.border_x >> ss, bdy = a.border_y >> ss;
    const int fxt = filter_table(b.filter_x, pbw), fyt = filter_table(b.filter_y, pbh);
    const int qx = clamped_mv(r ? b.mv1_x : b.mv0_x, b.x, bw, a.width, ss);
    const int qy = clamped_mv(r ? b.mv1_y : b.mv0_y, b.y, bh, a.height, ss);
    const int phx = qx & 15, phy = qy & 15, mode = (phx ? kHorz : 0) | (phy ? kVert : 0);
    const int sx = px + (qx >> 4) + sl.ox, sy = py + (qy >> 4) + sl.oy;
    tile_pass<T>((const T *)rp.plane[p], rp.stride[p], -bdx, pw + bdx - 1, -bdy, ph + bdy - 1, sx, sy, twl, thl, mode,
                 kInterpFilters[fxt][phx], kInterpFilters[fyt][phy], cr, win, im, li, lps, emit);
}

// The host side of a tile kernel's batch entry (Args: refs, blocks, items, pred, n_items, width, height, border_x, border_y,
// bd): the shared checks, the item lists, the metadata, the launches.  block_ok(b): the entry's own clauses.  later(b): the
// block's chroma tiles go to a second list, launched behind the first in the same stream.  prepare(a, has_later): the
// entry's own kernel arguments; 0 or an error code.
template <typename Args, typename Block, typename Ok, typename Later, typename Prepare>
int tile_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x, int32_t border_y, const Block *blocks,
               int32_t n_blocks, int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream, void (*k8)(Args),
               void (*k16)(Args), Ok block_ok, Later later, Prepare prepare) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!batch_args_ok(s, refs, n_refs, blocks, n_blocks, bit_depth, pred, border_x, border_y)) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    const int nplanes = chroma ? 3 : 1;
    if (!check_planes(refs, n_refs, pred, width, border_x, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    ItemBuilder list[2];
    for (int i = 0; i < n_blocks; i++) {
        const Block &b = blocks[i]; // ref0 .. filter_y: what ref_pass reads of either block type
        if (!check_block_rect(b.x, b.y, b.w_log2, b.h_log2, 4, width, height) || b.ref0 >= n_refs || b.ref1 >= n_refs ||
            b.filter_x > 3 || b.filter_y > 3 || !block_ok(b))
            return SVTGPU_ERR_INVALID_ARG;
        for (int p = 0; p < nplanes; p++) list[p && later(b)].add_plane((uint32_t)i, p, b.w_log2, b.h_log2);
    }
    if (!n_blocks) return SVTGPU_OK;
    Args a;
    memset(&a, 0, sizeof a);
    if (int rc = prepare(a, !list[1].items.empty())) return rc;
    hipStream_t      st = pick_stream(ctx, stream);
    const size_t     n[2] = {list[0].items.size(), list[1].items.size()};
    const MetaLayout lay((size_t)n_refs, (size_t)n_blocks, sizeof(Block), n[0] + n[1], sizeof(CompItem));
    uint8_t         *dm;
    if (int rc = meta_upload(s, lay, refs, blocks, st, &dm, list[0].items.data(), n[0] * sizeof(CompItem), list[1].items.data()))
        return rc;
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const Block *)(dm + lay.o_blk), a.pred = *pred;
    a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y, a.bd = bit_depth;
    for (int pass = 0; pass < 2; pass++) {
        if (!n[pass]) continue;
        a.items = (const CompItem *)(dm + lay.o_item) + (pass ? n[0] : 0), a.n_items = (int32_t)n[pass];
        if (int rc = launch_by_depth(bit_depth, k8, k16, dim3((unsigned)((n[pass] + 3) / 4)), dim3(256), st, a)) return rc;
    }
    return SVTGPU_OK;
}

} // namespace compound_tile
