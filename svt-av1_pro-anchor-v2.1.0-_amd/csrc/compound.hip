// compound.hip — AV1 compound (two-reference) inter prediction on gfx950: svt_av1_jnt_convolve_{2d,x,y,2d_copy}_c and
// svt_av1_highbd_jnt_convolve_*_c (EbInterPrediction.c:503-677, :861-1040) behind eight RTCD shims, and the bi-predicted
// blocks of a picture (svt_aom_inter_prediction with is_compound = 1, COMPOUND_AVERAGE or COMPOUND_DISTWTD, translation,
// unscaled references; EbEncInterPrediction.c:4070) as one launch, svtgpu_compound_predict_batch.
//
// The tile machinery -- units, tile passes, one reference's pass of a block's tile -- is csrc/compound_tile.h, shared with
// masked_compound.hip; the items, the LDS budget and the entry's checks are csrc/pred_plan.h.  Here:
//   combine      reference 0's values stay in the lane's registers (the same lane owns the same units in both passes, at
//                most four of them); after reference 1's pass the lane averages or distance-weights, removes the offsets,
//                rounds, clips and stores four samples with one vector store.  CONV_BUF_TYPE never reaches global memory.
//   item list    the host builds it while it checks the blocks (it walks them anyway, and a device-side prefix over tile
//                counts would cost a second launch or a search per workgroup); the list travels in the state's metadata
//                buffer behind the plane descriptors and the blocks.
//   workgroup    four waves, four consecutive items; no workgroup barrier, no atomics: a wave's LDS slice is private and
//                its DS operations complete in order.
//
// Bounds.  Reference reads: coordinates clamped into [-border, size + border - 1] of the plane, which the entry's contract
// makes readable.  Predictor writes: inside the block, which the entry checked against the state's picture area and the
// strides against that.  blocks[] and refs[] indices are checked on the host.  LDS: pred_plan.h.
#include "compound_tile.h"
#include "compound_weights.h"

static_assert(sizeof(SvtGpuCompoundBlock) == 32, "SvtGpuCompoundBlock is 32 bytes");

using namespace compound_tile;

namespace {

// ---------------------------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------------------------
struct CompArgs {
    const SvtGpuTfPlanes      *refs;   // [n_refs]
    const SvtGpuCompoundBlock *blocks; // [n_blocks]
    const CompItem            *items;  // [n_items]
    SvtGpuTfPlanes             pred;
    int32_t                    n_items, width, height, border_x, border_y, bd;
};

template <typename T>
__global__ __launch_bounds__(256) void compound_kernel(const CompArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds_all[4 * kWaveLds];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it = blockIdx.x * 4 + wave;
    if (it >= a.n_items) return;
    const CompItem &item = a.items[it];
    const int twl = item.tw_log2, thl = item.th_log2, tw = 1 << twl, th = 1 << thl;
    const int ul = twl + thl - 2, lpl = ul < 6 ? ul : 6, lps = 1 << lpl, slot = lane >> lpl, li = lane & (lps - 1);
    if (slot >= item.nslots) return;
    const CompSlot            sl = item.slot[slot];
    const SvtGpuCompoundBlock b  = a.blocks[sl.blk];
    uint16_t *win = lds_all + wave * kWaveLds + slot * ((th + 7) * (tw + 8));
    int16_t  *im  = (int16_t *)(lds_all + wave * kWaveLds + kWinCap) + slot * ((th + 7) * tw);

    const int    p = sl.plane, ss = p > 0;
    // the block's origin in the plane: chroma at ((x >> 3) << 3) / 2 (EbEncInterPrediction.c:4269)
    const int    px = ss ? ((b.x >> 3) << 3) >> 1 : b.x, py = ss ? ((b.y >> 3) << 3) >> 1 : b.y;
    const Rounds cr = {3, 7, a.bd}; // get_conv_params_no_round(is_compound = 1) at 8 and 10 bits
    typedef typename Vec4<T>::type V4;
    // the plane by selects, not by a lane-varying index into the kernel arguments (that would put them in scratch)
    void *const pplane  = p == 0 ? a.pred.plane[0] : p == 1 ? a.pred.plane[1] : a.pred.plane[2];
    const int   pstride = p == 0 ? a.pred.stride[0] : p == 1 ? a.pred.stride[1] : a.pred.stride[2];
    T          *dst = (T *)pplane + (size_t)(py + sl.oy) * pstride + px + sl.ox;
    u16x4 first[4];
    for (int r = 0; r < 2; r++) {
        ref_pass<T>(a, b, sl, r, px, py, twl, thl, cr, win, im, li, lps,
                     [&](int i, int y, int x4, const int res[4]) __attribute__((always_inline)) {
                         if (r == 0) {
                             first[i] = (u16x4){(uint16_t)res[0], (uint16_t)res[1], (uint16_t)res[2], (uint16_t)res[3]};
                         } else {
                             V4 o;
#pragma unroll
                             for (int j = 0; j < 4; j++)
                                 o[j] = (T)compound_average(first[i][j], res[j], b.dist_wtd, b.fwd_offset, b.bck_offset, 3, 7, a.bd);
                             *(V4 *)(dst + (size_t)y * pstride + x4) = o;
                         }
                     });
    }
}

// ---------------------------------------------------------------------------------------------
// the shims' kernel: src is the staged (h + 7) x (w + 7) window (origin at (3, 3)); conv the packed w x h CONV_BUF_TYPE
// block (written when do_average == 0, read otherwise); dst the packed w x h pixel block.  One wave per tile.
// ---------------------------------------------------------------------------------------------
struct JntArgs {
    const void    *src;
    uint16_t      *conv;
    void          *dst;
    const int16_t *taps; // fx[8], fy[8]
    int32_t        w, h, mode, do_average, dist_wtd, fwd, bck;
    Rounds         cr;
};
template <typename T>
__global__ __launch_bounds__(64) void jnt_block_kernel(const JntArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[kWaveLds];
    const int twl = 31 - __clz(a.w < kTile ? a.w : kTile), thl = 31 - __clz(a.h < kTile ? a.h : kTile);
    const int tw = 1 << twl, th = 1 << thl, ul = twl + thl - 2, lps = ul < 6 ? 1 << ul : 64, li = (int)threadIdx.x;
    if (li >= lps) return;
    const int tx = blockIdx.x * tw, ty = blockIdx.y * th, ws = a.w + 7;
    typedef typename Vec4<T>::type V4;
    // the window is the whole plane here: size (w + 1) x (h + 1) with a border of 3 spans columns -3 .. w + 3
    tile_pass<T>((const T *)a.src + 3 * ws + 3, ws, -3, a.w + 3, -3, a.h + 3, tx, ty, twl, thl, a.mode, a.taps, a.taps + 8, a.cr,
                 lds, (int16_t *)(lds + kWinCap), li, lps, [&](int, int y, int x4, const int res[4]) __attribute__((always_inline)) {
                     uint16_t *c = a.conv + (size_t)(ty + y) * a.w + tx + x4;
                     if (!a.do_average) {
                         *(u16x4 *)c = (u16x4){(uint16_t)res[0], (uint16_t)res[1], (uint16_t)res[2], (uint16_t)res[3]};
                     } else {
                         const u16x4 f = *(const u16x4 *)c;
                         V4          o;
#pragma unroll
                         for (int j = 0; j < 4; j++)
                             o[j] = (T)compound_average(f[j], res[j], a.dist_wtd, a.fwd, a.bck, a.cr.r0, a.cr.r1, a.cr.bd);
                         *(V4 *)((T *)a.dst + (size_t)(ty + y) * a.w + tx + x4) = o;
                     }
                 });
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename T>
void shim_jnt(int mode, const T *src, int src_stride, T *dst, int dst_stride, int w, int h, const int16_t *fx, const int16_t *fy,
              int round_0, int round_1, uint16_t *conv_dst, int conv_dst_stride, int do_average, int use_jnt_comp_avg,
              int fwd_offset, int bck_offset, int bd) {
    if (!src || !conv_dst || (do_average && !dst) || !size_ok(w, 4) || !size_ok(h, 4) || ((mode & kHorz) && !fx) ||
        ((mode & kVert) && !fy) || (sizeof(T) == 1 ? bd != 8 : (bd != 10 && bd != 12)) || round_0 < 0 || round_0 > 7 ||
        round_1 < 0 || round_1 > 7 || conv_dst_stride < w)
        svtgpu_fatal("svtgpu compound convolve shim: bad arguments");
    const int    ws = w + 7, hs = h + 7;
    const size_t conv = (size_t)w * h * sizeof(uint16_t), out = (size_t)w * h * sizeof(T);
    Carver       c; // the window at 0, then the taps, conv_dst and the pixels
    c((size_t)ws * hs * sizeof(T));
    const size_t o_taps = c(32), o_conv = c(conv), o_out = c(out);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t *const hb = sg.h, *const d = sg.d;
    T           *hw = (T *)hb;
    // what the reference's C reads of src, and nothing else (as the single-reference shims)
    memset(hb, 0, o_conv);
    const int y0 = (mode & kVert) ? -3 : 0, y1 = (mode & kVert) ? h + 4 : h, x0 = (mode & kHorz) ? -3 : 0,
              x1 = (mode & kHorz) ? w + 4 : w;
    for (int y = y0; y < y1; y++)
        memcpy(hw + (size_t)(y + 3) * ws + x0 + 3, src + (ptrdiff_t)y * src_stride + x0, (size_t)(x1 - x0) * sizeof(T));
    if (fx) memcpy(hb + o_taps, fx, 16);
    if (fy) memcpy(hb + o_taps + 16, fy, 16);
    size_t up = o_conv;
    if (do_average) {
        pack_rows(hb + o_conv, conv_dst, (ptrdiff_t)conv_dst_stride * 2, (size_t)w * 2, h);
        up = o_conv + conv;
    }
    HIP_OR_DIE(hipMemcpyAsync(d, hb, up, hipMemcpyHostToDevice, st));
    JntArgs a;
    memset(&a, 0, sizeof a);
    a.src = d, a.conv = (uint16_t *)(d + o_conv), a.dst = d + o_out, a.taps = (const int16_t *)(d + o_taps);
    a.w = w, a.h = h, a.mode = mode, a.do_average = do_average, a.dist_wtd = use_jnt_comp_avg, a.fwd = fwd_offset,
    a.bck = bck_offset, a.cr = {round_0, round_1, bd};
    const dim3 grid((unsigned)((w + kTile - 1) / kTile), (unsigned)((h + kTile - 1) / kTile));
    hipLaunchKernelGGL(jnt_block_kernel<T>, grid, dim3(64), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    const size_t o_back = do_average ? o_out : o_conv, n_back = do_average ? out : conv;
    HIP_OR_DIE(hipMemcpyAsync(hb + o_back, d + o_back, n_back, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    if (do_average)
        unpack_rows(dst, (ptrdiff_t)dst_stride * sizeof(T), hb + o_out, (size_t)w * sizeof(T), h);
    else
        unpack_rows(conv_dst, (ptrdiff_t)conv_dst_stride * 2, hb + o_conv, (size_t)w * 2, h);
}

} // namespace

extern "C" int svtgpu_dist_wtd_weights(int32_t d0, int32_t d1, int32_t order_idx, int32_t *fwd_offset, int32_t *bck_offset) {
    return compound_weights::select(d0, d1, order_idx, fwd_offset, bck_offset) ? SVTGPU_OK : SVTGPU_ERR_INVALID_ARG;
}

extern "C" int svtgpu_compound_predict_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                             int32_t border_y, const SvtGpuCompoundBlock *blocks, int32_t n_blocks,
                                             int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream) {
    return tile_batch<CompArgs>(
        s, refs, n_refs, border_x, border_y, blocks, n_blocks, bit_depth, chroma, pred, stream, compound_kernel<uint8_t>,
        compound_kernel<uint16_t>, [](const SvtGpuCompoundBlock &b) { return dist_wtd_ok(b.dist_wtd, b.fwd_offset, b.bck_offset); },
        [](const SvtGpuCompoundBlock &) { return false; }, [](CompArgs &, bool) { return 0; });
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous.  svtgpu_rtcd.h's adapters, compiled inside the encoder, select the kernel rows
// from the reference's InterpFilterParams and spell its ConvolveParams out.
// ---------------------------------------------------------------------------------------------
#define SVTGPU_JNT_SHIM(name, mode)                                                                                          \
    extern "C" void svtgpu_av1_jnt_convolve_##name(                                                                          \
        const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w, int32_t h,                      \
        const int16_t *filter_x, const int16_t *filter_y, int32_t round_0, int32_t round_1, uint16_t *conv_dst,              \
        int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset) {     \
        shim_jnt<uint8_t>(mode, src, src_stride, dst, dst_stride, w, h, filter_x, filter_y, round_0, round_1, conv_dst,      \
                          conv_dst_stride, do_average, use_jnt_comp_avg, fwd_offset, bck_offset, 8);                         \
    }                                                                                                                        \
    extern "C" void svtgpu_av1_highbd_jnt_convolve_##name(                                                                   \
        const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride, int32_t w, int32_t h,                    \
        const int16_t *filter_x, const int16_t *filter_y, int32_t round_0, int32_t round_1, uint16_t *conv_dst,              \
        int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset,       \
        int32_t bd) {                                                                                                        \
        shim_jnt<uint16_t>(mode, src, src_stride, dst, dst_stride, w, h, filter_x, filter_y, round_0, round_1, conv_dst,     \
                           conv_dst_stride, do_average, use_jnt_comp_avg, fwd_offset, bck_offset, bd);                       \
    }
SVTGPU_JNT_SHIM(2d, k2d)
SVTGPU_JNT_SHIM(x, kHorz)
SVTGPU_JNT_SHIM(y, kVert)
SVTGPU_JNT_SHIM(2d_copy, kCopy)
