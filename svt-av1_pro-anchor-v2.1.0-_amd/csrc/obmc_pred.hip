// obmc_pred.hip — AV1 OBMC prediction on gfx950: svt_aom_inter_prediction with is_compound = 0 and motion_mode =
// OBMC_CAUSAL (EbEncInterPrediction.c:4070, :4507; av1_inter_prediction_obmc :3774) for a list of blocks as one launch,
// svtgpu_obmc_predict_batch.  With empty neighbour lists it is the single-reference predictor of a block list.
//
// The rules -- masks, blend, strip geometry, taps, clamp, list validation, a span's rectangle in a tile -- are
// csrc/obmc_plan.h; the wave items are pred_plan.h's (one tile of at most 32 x 32 of one plane of one block, small tiles
// gathered); the window staging is compound_tile.h's.  Here:
//   region pass  (sr_region.h, shared with interintra.hip) one reference over a rectangle of the tile: the lanes of the tile's slot stage the rectangle's window, run
//                the horizontal filter into the intermediate when both phases are set, and each lane finishes those of its
//                own units (four adjacent samples; the same lane owns the same units in every pass) that lie inside the
//                rectangle, as pixels, by the convolve_*_sr function of the phases (EbInterPrediction.c:320-427, :679-786).
//   a tile       the block's own pass over the whole tile into registers; then one pass per above span and one per left
//                span that touches the tile, over the blended part of the strip only, blended into the registers (above
//                before left, AOM_BLEND_A64 each); then one vector store per unit.  pred is never read.
//   workgroup    four waves, four consecutive items; no workgroup barrier, no atomics.  The slots of a gathered item hold
//                different blocks: their pass counts differ, so the pass loops run under the lanes' own conditions and every
//                LDS index stays inside the slot's own slice.
//
// Bounds.  Reference reads: coordinates clamped into [-border, size + border - 1] of the plane.  Predictor writes: inside
// the block, which the entry checked against the picture area.  blocks[], refs[] and nb[] indices are checked on the host.
// LDS: a rectangle is no larger than its tile, so its window and intermediate fit the slot's slice (pred_plan.h).
#include "sr_region.h"

static_assert(sizeof(SvtGpuObmcNeighbour) == 8 && sizeof(SvtGpuObmcBlock) == 96, "SvtGpuObmcBlock is 96 bytes");

using namespace compound_tile;
using namespace obmc_plan;
using namespace sr_region;

namespace {

struct ObmcArgs {
    const SvtGpuTfPlanes  *refs;   // [n_refs]
    const SvtGpuObmcBlock *blocks; // [n_blocks]
    const CompItem        *items;  // [n_items]
    SvtGpuTfPlanes         pred;
    int32_t                n_items, width, height, border_x, border_y, bd;
};

// The region passes of the spans of direction dir (0 above, 1 left) that touch the tile of slot sl: the span's reference, MV,
// filter kinds, tap rule and clamp by obmc_plan.h.  emit(i, y, x4, res, depth): (y, x4) in the tile, depth the mask's length.
template <typename T, typename Args, typename Emit>
__device__ __forceinline__ void span_passes(const Args &a, const SvtGpuObmcBlock *b, const CompSlot &sl, int dir, int gx, int gy,
                                            int twl, int thl, uint16_t *win, int16_t *im, int li, int lps, Emit emit) {
    const int p = sl.plane, ss = p > 0, bx = b->x, by = b->y, bw = 1 << b->w_log2, bh = 1 << b->h_log2;
    const int n = dir ? b->n_left : b->n_above;
    for (int k = 0; k < n; k++) {
        const SvtGpuObmcNeighbour nb = b->nb[4 * dir + k];
        Rect r;
        int  depth;
        if (!span_rect(dir, bw, bh, ss, nb.rel, nb.size, sl.ox, sl.oy, 1 << twl, 1 << thl, &r, &depth)) continue;
        const int along = strip_size_along(nb.size, ss);
        int       qx, qy, fxt, fyt;
        if (dir == 0) {
            qx = strip_mv_along(nb.mv_x, bx, nb.rel, nb.size, a.width, ss), qy = strip_mv_across(nb.mv_y, by, bh, a.height, ss);
            fxt = filter_table(nb.filters & 15, along), fyt = filter_table(nb.filters >> 4, pred_depth(bh, ss));
        } else {
            qx = strip_mv_across(nb.mv_x, bx, bw, a.width, ss), qy = strip_mv_along(nb.mv_y, by, nb.rel, nb.size, a.height, ss);
            fxt = filter_table(nb.filters & 15, pred_depth(bw, ss)), fyt = filter_table(nb.filters >> 4, along);
        }
        region_pass<T>(a, nb.ref, p, qx, qy, fxt, fyt, gx, gy, r, twl, thl, win, im, li, lps,
                       [&](int i, int y, int x4, const int res[4]) __attribute__((always_inline)) { emit(i, y, x4, res, depth); });
    }
}

template <typename T>
__global__ __launch_bounds__(256) void obmc_pred_kernel(const ObmcArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds_all[4 * kWaveLds];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it = blockIdx.x * 4 + wave;
    if (it >= a.n_items) return;
    const CompItem &item = a.items[it];
    const int twl = item.tw_log2, thl = item.th_log2, tw = 1 << twl, th = 1 << thl;
    const int ul = twl + thl - 2, lpl = ul < 6 ? ul : 6, lps = 1 << lpl, slot = lane >> lpl, li = lane & (lps - 1);
    if (slot >= item.nslots) return;
    const CompSlot         sl = item.slot[slot];
    const SvtGpuObmcBlock *b  = a.blocks + sl.blk;
    uint16_t *win = lds_all + wave * kWaveLds + slot * ((th + 7) * (tw + 8));
    int16_t  *im  = (int16_t *)(lds_all + wave * kWaveLds + kWinCap) + slot * ((th + 7) * tw);

    const int p = sl.plane, ss = p > 0, bx = b->x, by = b->y, bw = 1 << b->w_log2, bh = 1 << b->h_log2;
    const int gx = (bx >> ss) + sl.ox, gy = (by >> ss) + sl.oy; // x and y are multiples of 8: chroma at x / 2, y / 2
    typedef typename Vec4<T>::type V4;
    void *const pplane  = p == 0 ? a.pred.plane[0] : p == 1 ? a.pred.plane[1] : a.pred.plane[2];
    const int   pstride = p == 0 ? a.pred.stride[0] : p == 1 ? a.pred.stride[1] : a.pred.stride[2];
    T          *dst = (T *)pplane + (size_t)gy * pstride + gx;

    // the block's own prediction
    u16x4 own[4];
    region_pass<T>(a, b->ref, p, clamped_mv(b->mv_x, bx, bw, a.width, ss), clamped_mv(b->mv_y, by, bh, a.height, ss),
                   filter_table(b->filter_x, bw >> ss), filter_table(b->filter_y, bh >> ss), gx, gy, Rect{0, 0, tw, th}, twl, thl,
                   win, im, li, lps, [&](int i, int, int, const int res[4]) __attribute__((always_inline)) {
                       own[i] = (u16x4){(uint16_t)res[0], (uint16_t)res[1], (uint16_t)res[2], (uint16_t)res[3]};
                   });
    // the above spans, then the left spans; the mask is indexed by the sample's offset across the edge in the block's plane
    for (int dir = 0; dir < 2; dir++)
        span_passes<T>(a, b, sl, dir, gx, gy, twl, thl, win, im, li, lps,
                       [&](int i, int y, int x4, const int res[4], int depth) __attribute__((always_inline)) {
#pragma unroll
                           for (int j = 0; j < 4; j++) {
                               const int pos = dir ? sl.ox + x4 + j : sl.oy + y;
                               if (pos < depth) own[i][j] = (uint16_t)blend_a64(kMasks[depth + pos], own[i][j], res[j]);
                           }
                       });
    const int gl = twl - 2, units = 1 << ul;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = li + i * lps;
        if (u < units) {
            const int y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
            *(V4 *)(dst + (size_t)y * pstride + x4) = (V4){(T)own[i][0], (T)own[i][1], (T)own[i][2], (T)own[i][3]};
        }
    }
}

// ---------------------------------------------------------------------------------------------
// wsrc / mask of calc_target_weighted_pred (EbEncInterPrediction.c:1767-1827) with
// svt_av1_calc_target_weighted_pred_{above,left}_c (:1592-1649): luma, 8 bits.  The same items and the same span passes as the
// predictor, without the block's own pass; a lane holds wsrc and mask of its units in registers through the four steps and
// stores each entry once.
// ---------------------------------------------------------------------------------------------
struct WsrcArgs {
    const SvtGpuTfPlanes  *refs;
    const SvtGpuObmcBlock *blocks;
    const CompItem        *items;
    const uint8_t         *src;
    int32_t               *wm;
    int32_t                src_stride, n_items, width, height, border_x, border_y, bd;
};
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void obmc_wsrc_kernel(const WsrcArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds_all[4 * kWaveLds];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it = blockIdx.x * 4 + wave;
    if (it >= a.n_items) return;
    const CompItem &item = a.items[it];
    const int twl = item.tw_log2, thl = item.th_log2, tw = 1 << twl, th = 1 << thl;
    const int ul = twl + thl - 2, lpl = ul < 6 ? ul : 6, lps = 1 << lpl, slot = lane >> lpl, li = lane & (lps - 1);
    if (slot >= item.nslots) return;
    const CompSlot         sl = item.slot[slot];
    const SvtGpuObmcBlock *b  = a.blocks + sl.blk;
    uint16_t *win = lds_all + wave * kWaveLds + slot * ((th + 7) * (tw + 8));
    int16_t  *im  = (int16_t *)(lds_all + wave * kWaveLds + kWinCap) + slot * ((th + 7) * tw);
    const int bw = 1 << b->w_log2, bh = 1 << b->h_log2, gx = b->x + sl.ox, gy = b->y + sl.oy;
    i32x4     ws[4], mk[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ws[i] = (i32x4){0, 0, 0, 0}, mk[i] = (i32x4){64, 64, 64, 64};
    span_passes<uint8_t>(a, b, sl, 0, gx, gy, twl, thl, win, im, li, lps,
                         [&](int i, int y, int x4, const int res[4], int depth) __attribute__((always_inline)) {
                             const int pos = sl.oy + y;
                             if (pos < depth) {
                                 const int m0 = kMasks[depth + pos];
#pragma unroll
                                 for (int j = 0; j < 4; j++) ws[i][j] = (64 - m0) * res[j], mk[i][j] = m0;
                             }
                         });
#pragma unroll
    for (int i = 0; i < 4; i++) ws[i] *= 64, mk[i] *= 64;
    span_passes<uint8_t>(a, b, sl, 1, gx, gy, twl, thl, win, im, li, lps,
                         [&](int i, int y, int x4, const int res[4], int depth) __attribute__((always_inline)) {
#pragma unroll
                             for (int j = 0; j < 4; j++) {
                                 const int pos = sl.ox + x4 + j;
                                 if (pos < depth) {
                                     const int m0 = kMasks[depth + pos];
                                     ws[i][j] = (ws[i][j] >> 6) * m0 + (res[j] << 6) * (64 - m0), mk[i][j] = (mk[i][j] >> 6) * m0;
                                 }
                             }
                         });
    const int gl = twl - 2, units = 1 << ul;
    int32_t  *wdst = a.wm + b->wm_offset;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = li + i * lps;
        if (u < units) {
            const int      y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
            const uint8_t *sp = a.src + (size_t)(gy + y) * a.src_stride + gx + x4;
            const int      off = (sl.oy + y) * bw + sl.ox + x4;
            i32x4          o;
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = (int)sp[j] * 4096 - ws[i][j];
            *(i32x4 *)(wdst + off) = o;
            *(i32x4 *)(wdst + bw * bh + off) = mk[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the blend shims' kernel: svt_aom_blend_a64_{v,h}mask (EbBlend_a64_mask.c:302, :350) and the highbd forms
// (C_DEFAULT/EbBlend_a64_mask_c.c:15, EbInterPrediction.c:2383) on packed w x h blocks; one sample per lane
// ---------------------------------------------------------------------------------------------
struct BlendArgs {
    const void    *src0, *src1;
    void          *dst;
    const uint8_t *mask;
    int32_t        w_log2, n, horizontal;
};
template <typename T>
__global__ __launch_bounds__(256) void blend_mask_kernel(const BlendArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int m = a.mask[a.horizontal ? i & ((1 << a.w_log2) - 1) : i >> a.w_log2];
    ((T *)a.dst)[i] = (T)blend_a64(m, ((const T *)a.src0)[i], ((const T *)a.src1)[i]);
}

template <typename T>
void shim_blend(int horizontal, T *dst, uint32_t dst_stride, const T *src0, uint32_t src0_stride, const T *src1,
                uint32_t src1_stride, const uint8_t *mask, int w, int h) {
    const int nm = horizontal ? w : h;
    bool      ok = dst && src0 && src1 && mask && size_ok(w, 1) && size_ok(h, 1) && (int64_t)dst_stride >= w &&
              (int64_t)src0_stride >= w && (int64_t)src1_stride >= w;
    for (int k = 0; ok && k < nm; k++) ok = mask[k] <= 64;
    if (!ok) svtgpu_fatal("svtgpu blend_a64 v/h mask shim: bad arguments");
    const size_t blk = (size_t)w * h * sizeof(T);
    Carver       c; // src0 at 0, then src1, the mask and the pixels
    c(blk);
    const size_t o1 = c(blk), om = c(128), oo = c(blk);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    // every read happens here, before anything is written: src0 / src1 may alias dst
    pack_rows(sg.h, src0, (ptrdiff_t)src0_stride * sizeof(T), (size_t)w * sizeof(T), h);
    pack_rows(sg.h + o1, src1, (ptrdiff_t)src1_stride * sizeof(T), (size_t)w * sizeof(T), h);
    memset(sg.h + om, 0, 128);
    memcpy(sg.h + om, mask, (size_t)nm);
    HIP_OR_DIE(hipMemcpyAsync(sg.d, sg.h, oo, hipMemcpyHostToDevice, st));
    BlendArgs a;
    memset(&a, 0, sizeof a);
    a.src0 = sg.d, a.src1 = sg.d + o1, a.mask = sg.d + om, a.dst = sg.d + oo;
    a.w_log2 = log2_of(w), a.n = w * h, a.horizontal = horizontal;
    hipLaunchKernelGGL(blend_mask_kernel<T>, dim3((unsigned)((w * h + 255) / 256)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(sg.h + oo, sg.d + oo, blk, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    unpack_rows(dst, (ptrdiff_t)dst_stride * sizeof(T), sg.h + oo, (size_t)w * sizeof(T), h);
}
inline void check_bd(int bd) {
    if (bd != 8 && bd != 10 && bd != 12) svtgpu_fatal("svtgpu highbd blend_a64 v/h mask shim: bad bit depth");
}

// the checks the two batch entries share: the state, the references (luma only without chroma), the blocks' geometry and lists
template <typename Ok>
int check_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x, int32_t border_y,
                const SvtGpuObmcBlock *blocks, int32_t n_blocks, int32_t bit_depth, int nplanes, ItemBuilder &list, int32_t *width,
                int32_t *height, SvtGpuContext **ctx, Ok block_ok) {
    int32_t blk_cols, nblk;
    svtgpu_tf_state_geometry(s, ctx, width, height, &blk_cols, &nblk);
    if (!ref_planes_ok(refs, n_refs, *width, border_x, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    for (int i = 0; i < n_blocks; i++) {
        const SvtGpuObmcBlock &b = blocks[i];
        if (!check_block_rect(b.x, b.y, b.w_log2, b.h_log2, 8, *width, *height) || !reserved_ok(b) || !lists_ok(b) || !block_ok(b))
            return SVTGPU_ERR_INVALID_ARG;
        for (int d = 0; d < 2; d++)
            for (int k = 0; k < (d ? b.n_left : b.n_above); k++) {
                const SvtGpuObmcNeighbour &nb = b.nb[4 * d + k];
                if (nb.ref >= n_refs || (nb.filters & 15) > 3 || (nb.filters >> 4) > 3) return SVTGPU_ERR_INVALID_ARG;
            }
        for (int p = 0; p < nplanes; p++) list.add_plane((uint32_t)i, p, b.w_log2, b.h_log2);
    }
    return SVTGPU_OK;
}

} // namespace

extern "C" int svtgpu_obmc_mask(int32_t length, const uint8_t **mask) {
    const uint8_t *m = mask_of(length);
    if (!mask || !m) return SVTGPU_ERR_INVALID_ARG;
    *mask = m;
    return SVTGPU_OK;
}

extern "C" int svtgpu_obmc_predict_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                         int32_t border_y, const SvtGpuObmcBlock *blocks, int32_t n_blocks, int32_t bit_depth,
                                         int32_t chroma, const SvtGpuTfPlanes *pred, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!batch_args_ok(s, refs, n_refs, blocks, n_blocks, bit_depth, pred, border_x, border_y)) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height;
    const int      nplanes = chroma ? 3 : 1;
    ItemBuilder    list;
    if (int rc = check_batch(s, refs, n_refs, border_x, border_y, blocks, n_blocks, bit_depth, nplanes, list, &width, &height, &ctx,
                             [&](const SvtGpuObmcBlock &b) { return b.ref < n_refs && b.filter_x <= 3 && b.filter_y <= 3; }))
        return rc;
    if (!pred_planes_ok(*pred, width, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    if (!n_blocks) return SVTGPU_OK;
    hipStream_t      st = pick_stream(ctx, stream);
    const size_t     n  = list.items.size();
    const MetaLayout lay((size_t)n_refs, (size_t)n_blocks, sizeof(SvtGpuObmcBlock), n, sizeof(CompItem));
    uint8_t         *dm;
    if (int rc = meta_upload(s, lay, refs, blocks, st, &dm, list.items.data(), n * sizeof(CompItem))) return rc;
    ObmcArgs a;
    memset(&a, 0, sizeof a);
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const SvtGpuObmcBlock *)(dm + lay.o_blk), a.pred = *pred;
    a.items = (const CompItem *)(dm + lay.o_item), a.n_items = (int32_t)n;
    a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y, a.bd = bit_depth;
    return launch_by_depth(bit_depth, obmc_pred_kernel<uint8_t>, obmc_pred_kernel<uint16_t>, dim3((unsigned)((n + 3) / 4)), dim3(256),
                           st, a);
}

extern "C" int svtgpu_obmc_weighted_src_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                              int32_t border_y, const void *src_luma, int32_t src_stride,
                                              const SvtGpuObmcBlock *blocks, int32_t n_blocks, int32_t *wm_dev, int32_t wm_count,
                                              void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!batch_args_ok(s, refs, n_refs, blocks, n_blocks, 8, wm_dev, border_x, border_y) || !src_luma || wm_count < 0 ||
        ((uintptr_t)wm_dev & 15))
        return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height;
    ItemBuilder    list;
    if (int rc = check_batch(s, refs, n_refs, border_x, border_y, blocks, n_blocks, 8, 1, list, &width, &height, &ctx,
                             [&](const SvtGpuObmcBlock &b) { // the block's own ref / mv / filters are not looked at
                                 return b.wm_offset >= 0 && !(b.wm_offset & 3) &&
                                        (int64_t)b.wm_offset + (2ll << (b.w_log2 + b.h_log2)) <= wm_count;
                             }))
        return rc;
    if (src_stride < width) return SVTGPU_ERR_INVALID_ARG;
    if (!n_blocks) return SVTGPU_OK;
    hipStream_t      st = pick_stream(ctx, stream);
    const size_t     n  = list.items.size();
    const MetaLayout lay((size_t)n_refs, (size_t)n_blocks, sizeof(SvtGpuObmcBlock), n, sizeof(CompItem));
    uint8_t         *dm;
    if (int rc = meta_upload(s, lay, refs, blocks, st, &dm, list.items.data(), n * sizeof(CompItem))) return rc;
    WsrcArgs a;
    memset(&a, 0, sizeof a);
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const SvtGpuObmcBlock *)(dm + lay.o_blk);
    a.items = (const CompItem *)(dm + lay.o_item), a.n_items = (int32_t)n, a.src = (const uint8_t *)src_luma, a.src_stride = src_stride;
    a.wm = wm_dev, a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y, a.bd = 8;
    hipLaunchKernelGGL(obmc_wsrc_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous, one stage reservation per call.  The _8bit forms take 16-bit samples behind a plain cast, as
// EbBlend_a64_mask.c:322-347 reads them (no CONVERT_TO_SHORTPTR).
// ---------------------------------------------------------------------------------------------
#define SVTGPU_BLEND_SHIMS(dir, horizontal)                                                                                        \
    extern "C" void svtgpu_aom_blend_a64_##dir(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,       \
                                               const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h) { \
        shim_blend<uint8_t>(horizontal, dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h);                        \
    }                                                                                                                              \
    extern "C" void svtgpu_aom_highbd_blend_a64_##dir##_16bit(uint16_t *dst, uint32_t dst_stride, const uint16_t *src0,             \
                                                              uint32_t src0_stride, const uint16_t *src1, uint32_t src1_stride,    \
                                                              const uint8_t *mask, int32_t w, int32_t h, int32_t bd) {             \
        check_bd(bd);                                                                                                              \
        shim_blend<uint16_t>(horizontal, dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h);                       \
    }                                                                                                                              \
    extern "C" void svtgpu_aom_highbd_blend_a64_##dir##_8bit(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0,                \
                                                             uint32_t src0_stride, const uint8_t *src1, uint32_t src1_stride,      \
                                                             const uint8_t *mask, int32_t w, int32_t h, int32_t bd) {              \
        check_bd(bd);                                                                                                              \
        shim_blend<uint16_t>(horizontal, (uint16_t *)dst, dst_stride, (const uint16_t *)src0, src0_stride,                          \
                             (const uint16_t *)src1, src1_stride, mask, w, h);                                                     \
    }
SVTGPU_BLEND_SHIMS(vmask, 0)
SVTGPU_BLEND_SHIMS(hmask, 1)
