// interp.hip — AV1 single-reference sub-pel interpolation on gfx950 and the motion compensation of the temporal filter
// built on it: svt_av1_convolve_{2d,x,y,2d_copy}_sr_c and svt_av1_highbd_convolve_*_sr_c (EbInterPrediction.c:320-427,
// :679-786) behind eight RTCD shims, and tf_64x64_inter_prediction / tf_32x32_inter_prediction
// (EbTemporalFiltering.c:2230-2580) for every (reference, 64x64 block) of a picture as one launch.
//
//   wave_region        one wave filters one region of at most 32x32 samples: it stages the (w + 7) x (h + 7) window of the
//                      reference into its own LDS slice once (every read coordinate clamped into the readable border),
//                      runs the horizontal pass into an int16 LDS intermediate of h + 7 rows and the vertical pass out of
//                      it.  The four forms are the reference's: 2-D (offset 1 << (bd + 6), round_0; offset
//                      1 << offset_bits, round_1, the two-term offset subtraction, the last rounding by `bits`), x-only
//                      (rounded by round_0, then by 7 - round_0), y-only (rounded once by 7), copy.  No workgroup
//                      barrier: the LDS slices are private to a wave, whose DS operations complete in order.
//   tf_predict_kernel  a workgroup owns one (reference, 64x64 block), a wave the 32x32 quarter idx_32x32 = the wave, as
//                      tf_frame_kernel maps them.  The wave walks its partition (its quarter of the 64x64 block, one
//                      32x32, or per 16x16 one block or four 8x8) and per sub-block filters luma and the half-size chroma
//                      blocks with the same MV.  The motion record is read with a wave-uniform index (scalar loads).
//   interp_block_kernel  the shims' kernel: one wave per 32x32 tile of the block, the same wave_region.
//
// MV handling restates compute_subpel_params' identity-scale branch (EbEncInterPrediction.c:3166-3177) with the edges of
// tf_*_inter_prediction (:2285-2297); the clamp is pred_plan::clamped_mv.
//
// Bounds: every reference read goes through clamp_i into [-border, size + border - 1] of the plane, which the entry's
// contract makes readable; predictor writes cover the 64-aligned area the entry checks the strides against; the motion
// index r * nblk + b < n_refs * nblk; LDS indices are below (rh + 7) * (rw + 7) <= 39 * 39 and (rh + 7) * rw <= 39 * 32.
#include "conv_device.h"
#include "interp_tables.h"
#include "svtgpu_internal.h"

static_assert(sizeof(SvtGpuTfMotion) == 368 && sizeof(SvtGpuTfMotion) % 16 == 0, "SvtGpuTfMotion is 368 bytes");

namespace {

using namespace conv_device;
using namespace pred_plan;

constexpr int kWin = kTile + 7;
enum { kCopy = 0, kHorz = 1, kVert = 2, k2d = 3 };

struct ConvRound {
    int32_t round_0, round_1, bd;
};
// one wave's LDS slice
template <typename T> struct WaveLds {
    T       win[kWin * kWin];
    int16_t im[kWin * kTile];
};

// One wave, one rw x rh region (powers of two, at most 32) whose top-left sample reads the reference at (sx, sy) of a
// pw x ph plane readable bx / by samples beyond each side.  fx / fy: wave-uniform pointers to the two 8-tap rows.
template <typename T>
__device__ __forceinline__ void wave_region(const T *__restrict__ ref, int stride, int pw, int ph, int bx, int by, int sx, int sy,
                                            int rw, int rh, const int16_t *fx, const int16_t *fy, int mode, ConvRound cr,
                                            T *__restrict__ dst, int dstride, WaveLds<T> *lds, int lane) {
    const int lw = 31 - __clz(rw), n = rw * rh;
    if (mode == kCopy) {
        for (int i = lane; i < n; i += 64) {
            const int y = i >> lw, x = i & (rw - 1);
            const int gx = clamp_i(sx + x, -bx, pw + bx - 1), gy = clamp_i(sy + y, -by, ph + by - 1);
            dst[(size_t)y * dstride + x] = ref[(ptrdiff_t)gy * stride + gx];
        }
        return;
    }
    const int ww = rw + 7, wh = rh + 7;
    // i / ww by a wave-uniform reciprocal: exact for ww in 8 .. 39 and i < 39 * 40 (the error is below i / 2^20 < 1 / ww)
    const int recip = (1 << 20) / ww + 1;
    for (int i = lane; i < ww * wh; i += 64) {
        const int y = (i * recip) >> 20, x = i - y * ww;
        const int gx = clamp_i(sx - 3 + x, -bx, pw + bx - 1), gy = clamp_i(sy - 3 + y, -by, ph + by - 1);
        lds->win[i] = ref[(ptrdiff_t)gy * stride + gx];
    }
    wave_lds_sync();
    if (mode == kHorz) {
        const int bits = 7 - cr.round_0;
        for (int i = lane; i < n; i += 64) {
            const int y = i >> lw, x = i & (rw - 1);
            const T  *p = lds->win + (y + 3) * ww + x;
            int       s = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) s += fx[k] * (int)p[k];
            s = round_shift(s, cr.round_0);
            dst[(size_t)y * dstride + x] = (T)clip_bd(round_shift(s, bits), cr.bd);
        }
    } else if (mode == kVert) {
        for (int i = lane; i < n; i += 64) {
            const int y = i >> lw, x = i & (rw - 1);
            const T  *p = lds->win + y * ww + x + 3;
            int       s = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) s += fy[k] * (int)p[k * ww];
            dst[(size_t)y * dstride + x] = (T)clip_bd(round_shift(s, 7), cr.bd);
        }
    } else {
        for (int i = lane; i < wh * rw; i += 64) {
            const int y = i >> lw, x = i & (rw - 1);
            const T  *p = lds->win + y * ww + x;
            int       s = 1 << (cr.bd + 6);
#pragma unroll
            for (int k = 0; k < 8; k++) s += fx[k] * (int)p[k];
            lds->im[i] = (int16_t)round_shift(s, cr.round_0);
        }
        wave_lds_sync();
        const int offset_bits = cr.bd + 14 - cr.round_0, bits = 14 - cr.round_0 - cr.round_1;
        const int sub = (1 << (offset_bits - cr.round_1)) + (1 << (offset_bits - cr.round_1 - 1));
        for (int i = lane; i < n; i += 64) {
            const int      y = i >> lw, x = i & (rw - 1);
            const int16_t *p = lds->im + (y << lw) + x;
            int            s = 1 << offset_bits;
#pragma unroll
            for (int k = 0; k < 8; k++) s += fy[k] * (int)p[k << lw];
            int res = round_shift(s, cr.round_1) - sub;
            if (sizeof(T) == 1) res = (int16_t)res; // the 8-bit function holds it in an int16 (:354), the highbd one in an int32
            dst[(size_t)y * dstride + x] = (T)clip_bd(round_shift(res, bits), cr.bd);
        }
    }
    wave_lds_sync(); // this region's LDS reads before the next region's stores
}

// ---------------------------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------------------------
struct PredPlanes { // one reference picture and its predictor picture
    const void *ref[3];
    void       *pred[3];
    int32_t     rstride[3], pstride[3];
};
struct PredArgs {
    const PredPlanes     *planes; // [n_refs]
    const SvtGpuTfMotion *motion; // [n_refs][nblk]
    int32_t               blk_cols, nblk, width, height, border_x, border_y, bd, tf_chroma;
};

// a prediction block of the reference's walk: origin (px, py) in luma samples of the picture, size b, MV in 1/8 luma sample;
// the wave filters the luma region (ox, oy) + rs x rs of it (the whole block but for the 64x64 one) and its chroma
template <typename T>
__device__ __forceinline__ void predict_block(const PredArgs &a, const PredPlanes &pl, int px, int py, int b, int mvx, int mvy,
                                              int ox, int oy, int rs, WaveLds<T> *lds, int lane) {
    const ConvRound cr = {3, 11, a.bd};
    const int       nplanes = a.tf_chroma ? 3 : 1;
    for (int p = 0; p < nplanes; p++) {
        const int ss = p > 0, bp = b >> ss;
        const int qx = clamped_mv(mvx, px, b, a.width, ss), qy = clamped_mv(mvy, py, b, a.height, ss);
        const int phx = qx & 15, phy = qy & 15;
        const int sx = (px >> ss) + (qx >> 4) + (ox >> ss), sy = (py >> ss) + (qy >> 4) + (oy >> ss);
        const int tab = bp <= 4 ? kInterpRegular4 : kInterpSharp; // MULTITAP_SHARP: the 4-tap table from w <= 4 / h <= 4
        const int mode = (phx ? kHorz : 0) | (phy ? kVert : 0);
        T *dst = (T *)pl.pred[p] + (size_t)((py + oy) >> ss) * pl.pstride[p] + ((px + ox) >> ss);
        wave_region<T>((const T *)pl.ref[p], pl.rstride[p], a.width >> ss, a.height >> ss, a.border_x >> ss, a.border_y >> ss,
                       sx, sy, rs >> ss, rs >> ss, kInterpFilters[tab][phx], kInterpFilters[tab][phy], mode, cr, dst,
                       pl.pstride[p], lds, lane);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void tf_predict_kernel(const PredArgs a) {
    __shared__ WaveLds<T> lds_all[4];
    const int  lane = threadIdx.x & 63, idx = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int  r = blockIdx.x / a.nblk, blk = blockIdx.x - r * a.nblk;
    const int  bx = (blk % a.blk_cols) * 64, by = (blk / a.blk_cols) * 64;
    WaveLds<T> *lds = &lds_all[idx];
    const PredPlanes     &pl = a.planes[r];
    const SvtGpuTfMotion &m  = a.motion[(size_t)r * a.nblk + blk];
    const int qx = (idx & 1) * 32, qy = (idx >> 1) * 32;
    if (m.use64) {
        predict_block<T>(a, pl, bx, by, 64, m.mv64_x, m.mv64_y, qx, qy, 32, lds, lane);
    } else if (!m.split32[idx]) {
        predict_block<T>(a, pl, bx + qx, by + qy, 32, m.mv32_x[idx], m.mv32_y[idx], 0, 0, 32, lds, lane);
    } else {
        for (int j = 0; j < 4; j++) {
            const int x16 = bx + qx + (j & 1) * 16, y16 = by + qy + (j >> 1) * 16, i16 = idx * 4 + j;
            if (!m.split16[i16]) {
                predict_block<T>(a, pl, x16, y16, 16, m.mv16_x[i16], m.mv16_y[i16], 0, 0, 16, lds, lane);
            } else {
                for (int k = 0; k < 4; k++)
                    predict_block<T>(a, pl, x16 + (k & 1) * 8, y16 + (k >> 1) * 8, 8, m.mv8_x[i16 * 4 + k], m.mv8_y[i16 * 4 + k],
                                     0, 0, 8, lds, lane);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the shims' kernel: src is the staged (h + 7) x (w + 7) window (origin at (3, 3)), dst packed w x h
// ---------------------------------------------------------------------------------------------
struct BlockArgs {
    const void *src;
    void       *dst;
    int32_t     w, h, mode;
    ConvRound   cr;
    int16_t     fx[8], fy[8];
};
template <typename T>
__global__ __launch_bounds__(64) void interp_block_kernel(const BlockArgs a) {
    __shared__ WaveLds<T> lds;
    const int tw = a.w < kTile ? a.w : kTile, th = a.h < kTile ? a.h : kTile;
    const int tx = blockIdx.x * tw, ty = blockIdx.y * th, ws = a.w + 7;
    // the window is the whole plane here: size (w + 1) x (h + 1) with a border of 3 spans columns -3 .. w + 3
    wave_region<T>((const T *)a.src + 3 * ws + 3, ws, a.w + 1, a.h + 1, 3, 3, tx, ty, tw, th, a.fx, a.fy, a.mode, a.cr,
                   (T *)a.dst + (size_t)ty * a.w + tx, a.w, &lds, (int)threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename T>
void shim_convolve(int mode, const T *src, int src_stride, T *dst, int dst_stride, int w, int h, const int16_t *fx,
                   const int16_t *fy, int round_0, int round_1, int bd) {
    if (!src || !dst || !size_ok(w, 2) || !size_ok(h, 2) || ((mode & kHorz) && !fx) || ((mode & kVert) && !fy) ||
        (sizeof(T) == 1 ? bd != 8 : (bd != 10 && bd != 12)) || round_0 < 0 || round_0 > 7 || round_1 < 0 ||
        (mode == k2d && (round_0 + round_1 > 14 || bd + 14 - round_0 - round_1 < 1)))
        svtgpu_fatal("svtgpu interpolation shim: bad arguments");
    const int    ws = w + 7, hs = h + 7;
    Carver       c;
    const size_t out = (size_t)w * h * sizeof(T), o_win = c((size_t)ws * hs * sizeof(T)), o_out = c(out);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t     *d  = sg.d;
    T           *hw = sg.host<T>(o_win);
    // what the reference's C reads of src, and nothing else: rows -3 .. h + 3 when it filters vertically (the y-only form
    // one more), columns -3 .. w + 4 when horizontally
    memset(hw, 0, o_out - o_win);
    const int y0 = (mode & kVert) ? -3 : 0, y1 = (mode & kVert) ? h + 4 : h, x0 = (mode & kHorz) ? -3 : 0,
              x1 = (mode & kHorz) ? w + 4 : w;
    for (int y = y0; y < y1; y++)
        memcpy(hw + (size_t)(y + 3) * ws + x0 + 3, src + (ptrdiff_t)y * src_stride + x0, (size_t)(x1 - x0) * sizeof(T));
    HIP_OR_DIE(hipMemcpyAsync(d + o_win, hw, o_out - o_win, hipMemcpyHostToDevice, st));
    BlockArgs a;
    memset(&a, 0, sizeof a);
    a.src = d + o_win, a.dst = d + o_out, a.w = w, a.h = h, a.mode = mode, a.cr = {round_0, round_1, bd};
    if (fx) memcpy(a.fx, fx, sizeof a.fx);
    if (fy) memcpy(a.fy, fy, sizeof a.fy);
    const dim3 grid((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile));
    hipLaunchKernelGGL(interp_block_kernel<T>, grid, dim3(64), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    uint8_t *ho = sg.h + o_out;
    HIP_OR_DIE(hipMemcpyAsync(ho, d + o_out, out, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    unpack_rows(dst, (ptrdiff_t)dst_stride * sizeof(T), ho, (size_t)w * sizeof(T), h);
}

} // namespace

extern "C" int svtgpu_interp_tables(const int16_t **tables, int32_t *n_tables) {
    if (!tables || !n_tables) return SVTGPU_ERR_INVALID_ARG;
    *tables = &kInterpFilters[0][0][0], *n_tables = kInterpTables;
    return SVTGPU_OK;
}

extern "C" int svtgpu_tf_predict_frame(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                       int32_t border_y, const SvtGpuTfMotion *motion, int32_t bit_depth, int32_t tf_chroma,
                                       const SvtGpuTfPlanes *pred, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!s || n_refs < 0 || (n_refs && (!refs || !motion || !pred)) || (bit_depth != 8 && bit_depth != 10) || border_x < 0 ||
        border_y < 0)
        return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    const int nplanes = tf_chroma ? 3 : 1; // without tf_chroma the chroma planes are neither checked nor touched
    if (!ref_planes_ok(refs, n_refs, width, border_x, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    for (int r = 0; r < n_refs; r++) // one predictor per reference, over the 64-aligned area
        if (!pred_planes_ok(pred[r], blk_cols * 64, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    if (!n_refs) return SVTGPU_OK;
    hipStream_t  st  = pick_stream(ctx, stream);
    const size_t off = (size_t)n_refs * sizeof(PredPlanes), nb = (size_t)n_refs * nblk * sizeof(SvtGpuTfMotion);
    uint8_t     *hm, *dm;
    if (int rc = svtgpu_tf_meta_begin(s, off + nb, &hm, &dm)) return rc;
    svtgpu_tf_predict_desc_fill(hm, refs, pred, n_refs);
    memcpy(hm + off, motion, nb);
    if (int rc = svtgpu_tf_meta_upload(s, off + nb, st)) return rc;
    return svtgpu_tf_predict_launch(s, dm, (const SvtGpuTfMotion *)(dm + off), n_refs, border_x, border_y, bit_depth, tf_chroma,
                                    st);
}

// tf_predict_kernel on descriptors and motion records that are on the device already (svtgpu_tf_compensate_filter_frame)
size_t svtgpu_tf_predict_desc_bytes() { return sizeof(PredPlanes); }
void   svtgpu_tf_predict_desc_fill(void *host, const SvtGpuTfPlanes *refs, const SvtGpuTfPlanes *pred, int n_refs) {
    PredPlanes *hp = (PredPlanes *)host;
    for (int r = 0; r < n_refs; r++)
        for (int p = 0; p < 3; p++) {
            hp[r].ref[p] = refs[r].plane[p], hp[r].rstride[p] = refs[r].stride[p];
            hp[r].pred[p] = pred[r].plane[p], hp[r].pstride[p] = pred[r].stride[p];
        }
}
int svtgpu_tf_predict_launch(SvtGpuTfState *s, const void *d_desc, const SvtGpuTfMotion *d_motion, int n_refs, int border_x,
                             int border_y, int bit_depth, int tf_chroma, hipStream_t st) {
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    PredArgs a;
    a.planes = (const PredPlanes *)d_desc, a.motion = d_motion;
    a.blk_cols = blk_cols, a.nblk = nblk, a.width = width, a.height = height;
    a.border_x = border_x, a.border_y = border_y, a.bd = bit_depth, a.tf_chroma = tf_chroma;
    return launch_by_depth(bit_depth, tf_predict_kernel<uint8_t>, tf_predict_kernel<uint16_t>, dim3((unsigned)(n_refs * nblk)),
                           dim3(256), st, a);
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous.  svtgpu_rtcd.h's adapters, compiled inside the encoder, select the kernel rows
// from the reference's InterpFilterParams and read round_0 / round_1 from its ConvolveParams.
// ---------------------------------------------------------------------------------------------
#define SVTGPU_INTERP_SHIM(name, mode)                                                                                       \
    extern "C" void svtgpu_av1_convolve_##name(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,   \
                                               int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,     \
                                               int32_t round_0, int32_t round_1) {                                         \
        shim_convolve<uint8_t>(mode, src, src_stride, dst, dst_stride, w, h, filter_x, filter_y, round_0, round_1, 8);     \
    }                                                                                                                      \
    extern "C" void svtgpu_av1_highbd_convolve_##name(const uint16_t *src, int32_t src_stride, uint16_t *dst,              \
                                                      int32_t dst_stride, int32_t w, int32_t h, const int16_t *filter_x,   \
                                                      const int16_t *filter_y, int32_t round_0, int32_t round_1,           \
                                                      int32_t bd) {                                                        \
        shim_convolve<uint16_t>(mode, src, src_stride, dst, dst_stride, w, h, filter_x, filter_y, round_0, round_1, bd);   \
    }
SVTGPU_INTERP_SHIM(2d_sr, k2d)
SVTGPU_INTERP_SHIM(x_sr, kHorz)
SVTGPU_INTERP_SHIM(y_sr, kVert)
SVTGPU_INTERP_SHIM(2d_copy_sr, kCopy)
