// interintra.hip — AV1 inter-intra prediction on gfx950: svt_aom_inter_prediction with is_interintra_used = 1
// (EbEncInterPrediction.c:4487; inter_intra_prediction :2548-2745) for a list of blocks as one launch,
// svtgpu_interintra_predict_batch; the four-mode luma distortion of inter_intra_search (EbModeDecision.c:275-478),
// svtgpu_interintra_mode_sse_batch, as a second instance of the same kernel; the host's smooth masks; and the RTCD shims of
// svt_aom_(highbd_)blend_a64_mask and of the intra predictors.
//
// The rules -- sizes, modes, edge preparation, DC, SMOOTH, the masks, the blend, the edge pool, validation -- are
// csrc/interintra_plan.h; the wave items are pred_plan.h's; the own pass is sr_region.h's.  A plane's block is at most 32 x 32,
// so it is one tile and a slot's tile origin is (0, 0).  A tile runs four steps:
//   own pass     the block's single-reference prediction of the plane into registers (region_pass over the whole tile).
//   edges        the slot's lanes bring the plane's prepared edges, above[tw] then left[th], as 16-bit samples into the first
//                tw + th elements of the slot's window slice: the own pass ends with wave_lds_sync(), so the window is free,
//                whatever the convolve form was.  DC: every lane sums the row and the column itself from 8-byte LDS reads of
//                one address for all lanes (at most 16 reads, 64 adds); a reduction over the slot's lanes would need
//                log2(lanes) cross-lane steps for each of the two sums under a lane count that differs between items, and
//                then a broadcast.  The division by w + h is a shift, or a shift and a multiplication (dc_divide).
//   blend        each lane, for its own units of four adjacent samples: the intra value (DC: the one value; V: one 8-byte
//                LDS read; H: left[y]; SMOOTH: both and the two corner samples, weights from kSmWeights), the mask value
//                (smooth: kIiWeights, 128 bytes of constant memory; wedge: wedge_masks.h's arithmetic, for chroma the
//                rounded mean of 2x2) and AOM_BLEND_A64 into the registers.
//   store        one vector store per unit; pred is never read.  The distortion instance keeps the inter prediction, loops
//                over the four modes with the smooth mask, and ends each with a butterfly sum over the slot's lanes; lane 0
//                of the slot stores the int64.
//   workgroup    four waves, four consecutive items; no workgroup barrier, no atomics.
//
// Bounds.  Reference reads: coordinates clamped into [-border, size + border - 1] of the plane.  Predictor writes: inside
// the block, which the entry checked against the picture area.  blocks[], refs[] and edge-pool indices (edge_offset + the
// plane's offset + [0, tw + th) < n_edges) are checked on the host; a prepared edge reads raw entries below n_top <= tw and
// n_left <= th only.  LDS: the edges take elements [0, tw + th) of the slot's window slice of (th + 7) * (tw + 8) elements, and
// tw + th <= 64 < 11 * 12.  The source plane is read inside the block.  sse[4 * blk + mode]: blk < n_blocks.
#include "sr_region.h" // before the plan headers: it brings the HIP runtime, whose qualifiers PRED_HD uses

#include "interintra_plan.h"

static_assert(sizeof(SvtGpuInterIntraBlock) == 32, "SvtGpuInterIntraBlock is 32 bytes");

using namespace compound_tile;
using namespace sr_region;
using namespace interintra_plan;

namespace {

struct IiArgs {
    const SvtGpuTfPlanes        *refs;   // [n_refs]
    const SvtGpuInterIntraBlock *blocks; // [n_blocks]
    const CompItem              *items;  // [n_items]
    const void                  *edges;  // the edge pool, in the sample type
    SvtGpuTfPlanes               pred;
    const void                  *src;    // the distortion instance: the source luma
    int64_t                     *sse;
    int32_t                      src_stride, n_items, width, height, border_x, border_y, bd;
};

// the intra values of the unit at row y, columns x4 .. x4 + 3 from the prepared edges in LDS (above at e, left at e + tw)
__device__ __forceinline__ void intra_unit(int mode, const uint16_t *e, int tw, int th, int dc, int y, int x4, int v[4]) {
    if (mode == kDcPred) {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = dc;
    } else if (mode == kHPred) {
        const int l = e[tw + y];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = l;
    } else {
        const u16x4 ab = *(const u16x4 *)(e + x4);
        if (mode == kVPred) {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = ab[j];
        } else {
            const int l = e[tw + y], below = e[tw + th - 1], right = e[tw - 1];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = smooth_value(ab[j], l, below, right, tw, th, y, x4 + j);
        }
    }
}

template <typename T, bool kSse>
__global__ __launch_bounds__(256) void interintra_kernel(const IiArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds_all[4 * kWaveLds];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it = blockIdx.x * 4 + wave;
    if (it >= a.n_items) return;
    const CompItem &item = a.items[it];
    const int twl = item.tw_log2, thl = item.th_log2, tw = 1 << twl, th = 1 << thl;
    const int ul = twl + thl - 2, lpl = ul < 6 ? ul : 6, lps = 1 << lpl, slot = lane >> lpl, li = lane & (lps - 1);
    if (slot >= item.nslots) return;
    const CompSlot               sl = item.slot[slot];
    const SvtGpuInterIntraBlock *b  = a.blocks + sl.blk;
    uint16_t *win = lds_all + wave * kWaveLds + slot * ((th + 7) * (tw + 8));
    int16_t  *im  = (int16_t *)(lds_all + wave * kWaveLds + kWinCap) + slot * ((th + 7) * tw);

    const int p = sl.plane, ss = p > 0, bx = b->x, by = b->y, bw = 1 << b->w_log2, bh = 1 << b->h_log2;
    const int gx = bx >> ss, gy = by >> ss; // x and y are multiples of 8; the tile is the plane's whole block

    // the block's own prediction
    u16x4 own[4];
    region_pass<T>(a, b->ref, p, clamped_mv(b->mv_x, bx, bw, a.width, ss), clamped_mv(b->mv_y, by, bh, a.height, ss),
                   filter_table(b->filter_x, bw >> ss), filter_table(b->filter_y, bh >> ss), gx, gy, Rect{0, 0, tw, th}, twl, thl,
                   win, im, li, lps, [&](int i, int, int, const int res[4]) __attribute__((always_inline)) {
                       own[i] = (u16x4){(uint16_t)res[0], (uint16_t)res[1], (uint16_t)res[2], (uint16_t)res[3]};
                   });
    // the prepared edges: above[tw], left[th]
    const T  *raw_above = (const T *)a.edges + b->edge_offset + edge_plane_offset(b->w_log2, b->h_log2, p), *raw_left = raw_above + tw;
    const int n_top = b->n_top[ss], n_left = b->n_left[ss];
    for (int k = li; k < tw + th; k += lps)
        win[k] = (uint16_t)(k < tw ? prepared_above(raw_above, raw_left, n_top, n_left, a.bd, k)
                                   : prepared_left(raw_above, raw_left, n_top, n_left, a.bd, k - tw));
    wave_lds_sync();
    const int variant = dc_variant(n_top, n_left);
    int       dc = 0;
    if (kSse || b->mode == kDcPred) {
        int sum_above = 0, sum_left = 0;
        for (int k = 0; k < tw; k += 4) {
            const u16x4 v = *(const u16x4 *)(win + k);
            sum_above += v[0] + v[1] + v[2] + v[3];
        }
        for (int k = 0; k < th; k += 4) {
            const u16x4 v = *(const u16x4 *)(win + tw + k);
            sum_left += v[0] + v[1] + v[2] + v[3];
        }
        dc = dc_value(variant, sum_above, sum_left, twl, thl, a.bd);
    }
    const int gl = twl - 2, units = 1 << ul;
    if (!kSse) {
        typedef typename Vec4<T>::type V4;
        void *const pplane  = p == 0 ? a.pred.plane[0] : p == 1 ? a.pred.plane[1] : a.pred.plane[2];
        const int   pstride = p == 0 ? a.pred.stride[0] : p == 1 ? a.pred.stride[1] : a.pred.stride[2];
        T          *dst = (T *)pplane + (size_t)gy * pstride + gx;
        const int   mode = b->mode, wedge = b->use_wedge;
        const wedge_masks::Plan wp = wedge_masks::plan(b->w_log2, b->h_log2, b->wedge_index, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int u = li + i * lps;
            if (u < units) {
                const int y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
                int       v[4];
                intra_unit(mode, win, tw, th, dc, y, x4, v);
                V4 o;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int m = wedge ? wedge_mask_plane(wp, ss, y, x4 + j) : smooth_mask(mode, twl, thl, y, x4 + j);
                    o[j] = (T)blend_a64(m, v[j], own[i][j]);
                }
                *(V4 *)(dst + (size_t)y * pstride + x4) = o;
            }
        }
    } else {
        const T *src = (const T *)a.src + (size_t)gy * a.src_stride + gx;
        u16x4    s[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int u = li + i * lps;
            if (u < units) {
                const T *sp = src + (size_t)(u >> gl) * a.src_stride + ((u & ((1 << gl) - 1)) << 2);
                s[i] = (u16x4){sp[0], sp[1], sp[2], sp[3]};
            }
        }
        for (int mode = 0; mode < kModes; mode++) {
            uint32_t acc = 0; // at most 16 samples of a lane, 1024 of a block: 1024 * 1023^2 < 2^32
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = li + i * lps;
                if (u < units) {
                    const int y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
                    int       v[4];
                    intra_unit(mode, win, tw, th, dc, y, x4, v);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int d = (int)s[i][j] - blend_a64(smooth_mask(mode, twl, thl, y, x4 + j), v[j], own[i][j]);
                        acc += (uint32_t)(d * d);
                    }
                }
            }
            // the slot's lanes are lps consecutive lanes from a multiple of lps, all active: the butterfly stays inside them
            for (int o = 1; o < lps; o <<= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
            if (li == 0) a.sse[4 * (size_t)sl.blk + mode] = (int64_t)acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the blend shims' kernel: svt_aom_blend_a64_mask / svt_aom_highbd_blend_a64_mask (EbBlend_a64_mask.c:201-299) on packed
// w x h blocks with a packed (w << subw) x (h << subh) mask; one sample per lane
// ---------------------------------------------------------------------------------------------
struct MaskBlendArgs {
    const void    *src0, *src1;
    void          *dst;
    const uint8_t *mask;
    int32_t        w_log2, n, subw, subh;
};
template <typename T>
__global__ __launch_bounds__(256) void blend_a64_mask_kernel(const MaskBlendArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int r = i >> a.w_log2, c = i & ((1 << a.w_log2) - 1), ms = 1 << (a.w_log2 + a.subw); // i < n: the mask index < n << (subw + subh)
    const uint8_t *mp = a.mask + (r << a.subh) * ms + (c << a.subw);
    int            m;
    if (a.subw && a.subh) m = (mp[0] + mp[ms] + mp[1] + mp[ms + 1] + 2) >> 2;
    else if (a.subw) m = blend_avg(mp[0], mp[1]);
    else if (a.subh) m = blend_avg(mp[0], mp[ms]);
    else m = mp[0];
    ((T *)a.dst)[i] = (T)blend_a64(m, ((const T *)a.src0)[i], ((const T *)a.src1)[i]);
}

template <typename T>
void shim_blend_mask(T *dst, uint32_t dst_stride, const T *src0, uint32_t src0_stride, const T *src1, uint32_t src1_stride,
                     const uint8_t *mask, uint32_t mask_stride, int w, int h, int subw, int subh) {
    bool ok = dst && src0 && src1 && mask && size_ok(w, 1) && size_ok(h, 1) && (int64_t)dst_stride >= w && (int64_t)src0_stride >= w &&
              (int64_t)src1_stride >= w && (subw == 0 || subw == 1) && (subh == 0 || subh == 1) && (int64_t)mask_stride >= ((int64_t)w << subw);
    const int mw = ok ? w << subw : 0, mh = ok ? h << subh : 0;
    for (int y = 0; ok && y < mh; y++)
        for (int x = 0; ok && x < mw; x++) ok = mask[(size_t)y * mask_stride + x] <= 64;
    if (!ok) svtgpu_fatal("svtgpu blend_a64_mask shim: bad arguments");
    const size_t blk = (size_t)w * h * sizeof(T);
    Carver       c; // src0 at 0, then src1, the mask and the pixels
    c(blk);
    const size_t o1 = c(blk), om = c((size_t)mw * mh), oo = c(blk);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    // every read happens here, before anything is written: src0 / src1 may alias dst
    pack_rows(sg.h, src0, (ptrdiff_t)src0_stride * sizeof(T), (size_t)w * sizeof(T), h);
    pack_rows(sg.h + o1, src1, (ptrdiff_t)src1_stride * sizeof(T), (size_t)w * sizeof(T), h);
    pack_rows(sg.h + om, mask, (ptrdiff_t)mask_stride, (size_t)mw, mh);
    HIP_OR_DIE(hipMemcpyAsync(sg.d, sg.h, oo, hipMemcpyHostToDevice, st));
    MaskBlendArgs a;
    memset(&a, 0, sizeof a);
    a.src0 = sg.d, a.src1 = sg.d + o1, a.mask = sg.d + om, a.dst = sg.d + oo;
    a.w_log2 = log2_of(w), a.n = w * h, a.subw = subw, a.subh = subh;
    hipLaunchKernelGGL(blend_a64_mask_kernel<T>, dim3((unsigned)((w * h + 255) / 256)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(sg.h + oo, sg.d + oo, blk, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    unpack_rows(dst, (ptrdiff_t)dst_stride * sizeof(T), sg.h + oo, (size_t)w * sizeof(T), h);
}

// ---------------------------------------------------------------------------------------------
// the intra shims' kernel: one w x h block from above[w] (at e) and left[h] (at e + w), one sample per lane; every lane sums
// the edges itself for the DC kinds
// ---------------------------------------------------------------------------------------------
struct IntraArgs {
    const void *edges;
    void       *dst;
    int32_t     w_log2, h_log2, kind, bd;
};
template <typename T>
__global__ __launch_bounds__(256) void intra_kernel(const IntraArgs a) {
    const int w = 1 << a.w_log2, h = 1 << a.h_log2, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const T  *e = (const T *)a.edges;
    const int r = i >> a.w_log2, c = i & (w - 1);
    int       v;
    if (a.kind == SVTGPU_INTRA_V) v = e[c];
    else if (a.kind == SVTGPU_INTRA_H) v = e[w + r];
    else if (a.kind == SVTGPU_INTRA_SMOOTH) v = smooth_value(e[c], e[w + r], e[w + h - 1], e[w - 1], w, h, r, c);
    else {
        int sa = 0, sl = 0;
        for (int k = 0; k < w; k++) sa += e[k];
        for (int k = 0; k < h; k++) sl += e[w + k];
        // a general size: plain division (dc_divide is for the ten plane sizes)
        v = a.kind == SVTGPU_INTRA_DC       ? (sa + sl + ((w + h) >> 1)) / (w + h)
            : a.kind == SVTGPU_INTRA_DC_TOP ? dc_value(kDcTop, sa, sl, a.w_log2, a.h_log2, a.bd)
            : a.kind == SVTGPU_INTRA_DC_LEFT ? dc_value(kDcLeft, sa, sl, a.w_log2, a.h_log2, a.bd)
                                             : base_value(a.bd);
    }
    ((T *)a.dst)[i] = (T)v;
}

template <typename T>
void shim_intra(T *dst, ptrdiff_t stride, const T *above, const T *left, int w, int h, int kind, int bd) {
    const bool side_ok = (w == 4 || w == 8 || w == 16 || w == 32) && (h == 4 || h == 8 || h == 16 || h == 32);
    if (!dst || !above || !left || !side_ok || kind < 0 || kind > SVTGPU_INTRA_SMOOTH || stride < w || (bd != 8 && bd != 10 && bd != 12))
        svtgpu_fatal("svtgpu intra predictor shim: bad arguments");
    const size_t blk = (size_t)w * h * sizeof(T);
    Carver       c;
    c((size_t)(w + h) * sizeof(T));
    const size_t oo = c(blk);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    memcpy(sg.h, above, (size_t)w * sizeof(T));
    memcpy(sg.h + (size_t)w * sizeof(T), left, (size_t)h * sizeof(T));
    HIP_OR_DIE(hipMemcpyAsync(sg.d, sg.h, (size_t)(w + h) * sizeof(T), hipMemcpyHostToDevice, st));
    IntraArgs a;
    memset(&a, 0, sizeof a);
    a.edges = sg.d, a.dst = sg.d + oo, a.w_log2 = log2_of(w), a.h_log2 = log2_of(h), a.kind = kind, a.bd = bd;
    hipLaunchKernelGGL(intra_kernel<T>, dim3((unsigned)((w * h + 255) / 256)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(sg.h + oo, sg.d + oo, blk, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    unpack_rows(dst, stride * (ptrdiff_t)sizeof(T), sg.h + oo, (size_t)w * sizeof(T), h);
}

// The two batch entries' host side: the checks, the items, the metadata with the edge pool behind it, the launch.  with_pred:
// the predict entry (pred, chroma, mode fields); otherwise the distortion entry (luma, src, sse).
int interintra_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x, int32_t border_y,
                     const SvtGpuInterIntraBlock *blocks, int32_t n_blocks, const void *edges, int32_t n_edges, int32_t bit_depth,
                     int nplanes, const SvtGpuTfPlanes *pred, const void *src, int32_t src_stride, int64_t *sse, void *stream) {
    const bool with_pred = pred != nullptr;
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!batch_args_ok(s, refs, n_refs, blocks, n_blocks, bit_depth, with_pred ? (const void *)pred : (const void *)sse, border_x, border_y) ||
        n_edges < 0 || (n_blocks && !edges))
        return SVTGPU_ERR_INVALID_ARG;
    const int bs = bit_depth > 8 ? 2 : 1;
    if (!with_pred && (!src || ((uintptr_t)src & (bs - 1)) || ((uintptr_t)sse & 7))) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    if (!ref_planes_ok(refs, n_refs, width, border_x, bit_depth, nplanes)) return SVTGPU_ERR_INVALID_ARG;
    if (with_pred ? !pred_planes_ok(*pred, width, bit_depth, nplanes) : src_stride < width) return SVTGPU_ERR_INVALID_ARG;
    ItemBuilder list;
    for (int i = 0; i < n_blocks; i++) {
        const SvtGpuInterIntraBlock &b = blocks[i];
        if (!check_block_rect(b.x, b.y, b.w_log2, b.h_log2, 8, width, height) || b.ref >= n_refs || !block_ok(b, nplanes, n_edges, with_pred))
            return SVTGPU_ERR_INVALID_ARG;
        for (int p = 0; p < nplanes; p++) list.add_plane((uint32_t)i, p, b.w_log2, b.h_log2);
    }
    if (!n_blocks) return SVTGPU_OK;
    hipStream_t      st = pick_stream(ctx, stream);
    const size_t     n  = list.items.size(), edge_bytes = (size_t)n_edges * bs;
    const MetaLayout lay((size_t)n_refs, (size_t)n_blocks, sizeof(SvtGpuInterIntraBlock), n, sizeof(CompItem));
    const size_t     o_edge = align16(lay.total), total = o_edge + edge_bytes;
    uint8_t         *hm, *dm;
    if (int rc = svtgpu_tf_meta_begin(s, total, &hm, &dm)) return rc;
    memcpy(hm, refs, lay.ref_bytes);
    memcpy(hm + lay.o_blk, blocks, lay.blk_bytes);
    memcpy(hm + lay.o_item, list.items.data(), lay.item_bytes);
    memcpy(hm + o_edge, edges, edge_bytes);
    if (int rc = svtgpu_tf_meta_upload(s, total, st)) return rc;
    IiArgs a;
    memset(&a, 0, sizeof a);
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const SvtGpuInterIntraBlock *)(dm + lay.o_blk);
    a.items = (const CompItem *)(dm + lay.o_item), a.n_items = (int32_t)n, a.edges = dm + o_edge;
    if (with_pred) a.pred = *pred;
    a.src = src, a.src_stride = src_stride, a.sse = sse;
    a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y, a.bd = bit_depth;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    return with_pred ? launch_by_depth(bit_depth, interintra_kernel<uint8_t, false>, interintra_kernel<uint16_t, false>, grid, block, st, a)
                     : launch_by_depth(bit_depth, interintra_kernel<uint8_t, true>, interintra_kernel<uint16_t, true>, grid, block, st, a);
}

} // namespace

extern "C" int svtgpu_interintra_smooth_mask(int32_t w, int32_t h, int32_t mode, uint8_t *mask) {
    if (!mask || mode < 0 || mode > 3 || !plane_size_ok(w, h)) return SVTGPU_ERR_INVALID_ARG;
    const int wl = log2_of(w), hl = log2_of(h);
    for (int r = 0; r < h; r++)
        for (int c = 0; c < w; c++) mask[r * w + c] = (uint8_t)smooth_mask(mode, wl, hl, r, c);
    return SVTGPU_OK;
}

extern "C" int svtgpu_interintra_predict_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                               int32_t border_y, const SvtGpuInterIntraBlock *blocks, int32_t n_blocks,
                                               const void *edges, int32_t n_edges, int32_t bit_depth, int32_t chroma,
                                               const SvtGpuTfPlanes *pred, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!pred) return SVTGPU_ERR_INVALID_ARG;
    return interintra_batch(s, refs, n_refs, border_x, border_y, blocks, n_blocks, edges, n_edges, bit_depth, chroma ? 3 : 1, pred, nullptr,
                            0, nullptr, stream);
}

extern "C" int svtgpu_interintra_mode_sse_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                                int32_t border_y, const SvtGpuInterIntraBlock *blocks, int32_t n_blocks,
                                                const void *edges, int32_t n_edges, int32_t bit_depth, const void *src_luma,
                                                int32_t src_stride, int64_t *sse_dev, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!sse_dev) return SVTGPU_ERR_INVALID_ARG;
    return interintra_batch(s, refs, n_refs, border_x, border_y, blocks, n_blocks, edges, n_edges, bit_depth, 1, nullptr, src_luma,
                            src_stride, sse_dev, stream);
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous, one stage reservation per call.  The highbd blend takes 16-bit samples behind a plain
// cast, as EbBlend_a64_mask.c:248-254 reads them (no CONVERT_TO_SHORTPTR).
// ---------------------------------------------------------------------------------------------
extern "C" void svtgpu_aom_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                          const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, uint32_t mask_stride, int w,
                                          int h, int subw, int subh) {
    shim_blend_mask<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subw, subh);
}
extern "C" void svtgpu_aom_highbd_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                                 const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask,
                                                 uint32_t mask_stride, int w, int h, int subw, int subh, int bd) {
    if (bd != 8 && bd != 10 && bd != 12) svtgpu_fatal("svtgpu highbd blend_a64_mask shim: bad bit depth");
    shim_blend_mask<uint16_t>((uint16_t *)dst, dst_stride, (const uint16_t *)src0, src0_stride, (const uint16_t *)src1, src1_stride, mask,
                              mask_stride, w, h, subw, subh);
}
extern "C" void svtgpu_aom_intra_predictor(uint8_t *dst, ptrdiff_t stride, const uint8_t *above, const uint8_t *left, int32_t w,
                                           int32_t h, int32_t kind) {
    shim_intra<uint8_t>(dst, stride, above, left, w, h, kind, 8);
}
extern "C" void svtgpu_aom_highbd_intra_predictor(uint16_t *dst, ptrdiff_t stride, const uint16_t *above, const uint16_t *left,
                                                  int32_t w, int32_t h, int32_t kind, int32_t bd) {
    shim_intra<uint16_t>(dst, stride, above, left, w, h, kind, bd);
}
