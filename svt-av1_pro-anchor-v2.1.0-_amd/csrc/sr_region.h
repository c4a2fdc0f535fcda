// sr_region.h — the single-reference region pass of the tile kernels (obmc_pred.hip, interintra.hip): one reference over a
// rectangle of a tile, finished as pixels by the convolve_*_sr function of the phases.  A tile, a unit, a slot and the window
// staging are compound_tile.h's; the rectangle is obmc_plan.h's.
#pragma once
#include "compound_tile.h"
#include "obmc_plan.h"

namespace sr_region {

using namespace compound_tile;
using obmc_plan::Rect;

// the 2-D form's horizontal pass (svt_av1_convolve_2d_sr_c :337-348) over a rectangle rw wide (a multiple of 4, at most 32):
// window rows 0 .. rh + 6 into im[rh + 7][rw]
__device__ __forceinline__ void horizontal_rows(const uint16_t *win, int16_t *im, int rw, int rh, const int fx[8], int bd, int li,
                                                int lps) {
    const int ws = rw + 8, g = rw >> 2, recip = (1 << 20) / g + 1; // u / g, exact for u < 39 * 8
    for (int u = li; u < (rh + 7) * g; u += lps) {
        const int    rr = (u * recip) >> 20, x4 = (u - rr * g) << 2;
        const u16x4 *p = (const u16x4 *)(win + rr * ws + x4);
        const u16x4  a = p[0], b = p[1], c = p[2];
        const int    s[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
        i16x4        o;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int sum = 1 << (bd + 6);
#pragma unroll
            for (int k = 0; k < 8; k++) sum += fx[k] * s[j + 1 + k];
            o[j] = (int16_t)round_shift(sum, 3);
        }
        *(i16x4 *)(im + rr * rw + x4) = o;
    }
}

// The four pixels of the unit at row y, columns x4 .. x4 + 3 of a rectangle rw wide, by the form's own C function with
// round_0 = 3, round_1 = 11 (get_conv_params_no_round, not compound, 8 and 10 bits): copy (:410-427), x (:383-408: rounded
// by round_0, then by 7 - round_0), y (:363-381: rounded once by 7), 2-D's vertical pass (:350-361: the two-term offset
// taken off, held in an int16 by the 8-bit function, the last rounding by 14 - 3 - 11 = 0 bits).
template <typename T>
__device__ __forceinline__ void sr_unit(int mode, const uint16_t *win, const int16_t *im, int rw, int y, int x4, const int fx[8],
                                        const int fy[8], int bd, int res[4]) {
    const int ws = rw + 8;
    if (mode == kCopy) {
        const u16x4 v = *(const u16x4 *)(win + (y + 3) * ws + x4 + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = v[j];
    } else if (mode == kHorz) {
        const u16x4 *p = (const u16x4 *)(win + (y + 3) * ws + x4);
        const u16x4  a = p[0], b = p[1], c = p[2];
        const int    s[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) sum += fx[k] * s[j + 1 + k];
            res[j] = clip_bd(round_shift(round_shift(sum, 3), 4), bd);
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
        for (int j = 0; j < 4; j++) res[j] = clip_bd(round_shift(sum[j], 7), bd);
    } else {
        const int offset_bits = bd + 11, sub = (1 << (offset_bits - 11)) + (1 << (offset_bits - 12));
        int       sum[4] = {1 << offset_bits, 1 << offset_bits, 1 << offset_bits, 1 << offset_bits};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const i16x4 v = *(const i16x4 *)(im + (y + k) * rw + x4);
#pragma unroll
            for (int j = 0; j < 4; j++) sum[j] += fy[k] * (int)v[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int v = round_shift(sum[j], 11) - sub;
            if (sizeof(T) == 1) v = (int16_t)v;
            res[j] = clip_bd(v, bd);
        }
    }
}

// One region pass for one lane: reference `ref` of plane p with the clamped MV (qx, qy) in 1/16 sample of the plane and the
// filter tables fxt / fyt, over rectangle r of the tile whose origin in the plane is (gx, gy).  emit(i, y, x4, res) for the
// lane's units u = li + i * lps inside r; (y, x4) in the tile.  r.w is a multiple of 4 from 4 to 32 and r.h at most 32
// (obmc_plan::span_rect; tests/obmc_plan_check.cpp holds it), so stage_window's groups per row g = (r.w + 8) / 4 are 3 .. 10
// and its and horizontal_rows' reciprocal divisions are exact.
template <typename T, typename Args, typename Emit>
__device__ __forceinline__ void region_pass(const Args &a, int ref, int p, int qx, int qy, int fxt, int fyt, int gx, int gy,
                                            Rect r, int twl, int thl, uint16_t *win, int16_t *im, int li, int lps, Emit emit) {
    const int             ss = p > 0;
    const SvtGpuTfPlanes &rp = a.refs[ref];
    const int pw = a.width >> ss, ph = a.height >> ss, bdx = a.border_x >> ss, bdy = a.border_y >> ss;
    const int phx = qx & 15, phy = qy & 15, mode = (phx ? kHorz : 0) | (phy ? kVert : 0);
    const int sx = gx + r.x0 + (qx >> 4), sy = gy + r.y0 + (qy >> 4);
    int       fx[8], fy[8];
    load_taps(kInterpFilters[fxt][phx], fx);
    load_taps(kInterpFilters[fyt][phy], fy);
    stage_window<T>((const T *)rp.plane[p], rp.stride[p], -bdx, pw + bdx - 1, -bdy, ph + bdy - 1, sx, sy, r.w, r.h, mode, win, li,
                    lps);
    wave_lds_sync();
    if (mode == k2d) horizontal_rows(win, im, r.w, r.h, fx, a.bd, li, lps);
    wave_lds_sync();
    const int gl = twl - 2, units = 1 << (twl + thl - 2);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = li + i * lps, y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
        if (u < units && y >= r.y0 && y < r.y0 + r.h && x4 >= r.x0 && x4 < r.x0 + r.w) {
            int res[4];
            sr_unit<T>(mode, win, im, r.w, y - r.y0, x4 - r.x0, fx, fy, a.bd, res);
            emit(i, y, x4, res);
        }
    }
    wave_lds_sync(); // this pass's LDS reads before the next pass's stores
}

} // namespace sr_region
