// masked_compound.hip — AV1 masked compound prediction on gfx950: COMPOUND_WEDGE and COMPOUND_DIFFWTD, the other two of
// the four inter-inter compound types.  svt_av1_build_compound_diffwtd_mask_d16_c (C_DEFAULT/EbInterPrediction_c.c:15-40),
// svt_aom_lowbd_blend_a64_d16_mask_c / svt_aom_highbd_blend_a64_d16_mask_c (EbBlend_a64_mask.c:34-195) behind three RTCD
// shims, the wedge masks of svt_av1_init_wedge_masks (csrc/wedge_masks.h), and the masked bi-predicted blocks of a picture
// (svt_aom_inter_prediction with a masked compound type: reference 1 through av1_make_masked_scaled_inter_predictor,
// EbEncInterPrediction.c:50-164) as svtgpu_masked_compound_predict_batch.
//
// The two reference passes of a tile are compound.hip's (ref_pass and tile_pass of csrc/compound_tile.h; the items and
// the entry's checks are csrc/pred_plan.h): reference 0's CONV_BUF_TYPE values stay
// in the lane's registers, and after reference 1's pass the lane blends its four samples by a 6-bit mask instead of
// averaging them.  Where the four mask values of a unit come from:
//   wedge, luma      wedge_masks::plan_value at the unit's four positions in the block: arithmetic on constants.
//   wedge, chroma    the rounded mean of the 2x2 mask values under each chroma sample (subw = subh = 1).
//   DIFFWTD, luma    from the lane's own two values: 38 + (|a - b| rounded by 14 - round_0 - round_1 + bd - 8) / 16, clamped
//                    to 64, complemented for DIFFWTD_38_INV.  With chroma on, the lane also stores the four bytes at the
//                    unit's luma position in the state's mask plane (one byte per luma sample of the picture).
//   DIFFWTD, chroma  the rounded 2x2 means of that plane under the unit: four 4-byte loads.
// A DIFFWTD chroma tile needs the mask of luma tiles that other workgroups compute, so the host puts those tiles in a
// second item list and launches the same kernel on it behind the first launch, in the same stream: the order of the two
// launches is the only synchronisation.  No flag, spin or other wait between workgroups.
//
// Bounds.  Reference reads and predictor writes as compound.hip.  Mask plane: a luma unit writes row b.y + oy + y, columns
// b.x + ox + x4 .. + 3, inside the block and so inside width x height (the entry checked the block); a chroma unit reads
// rows b.y + 2 (oy + y) .. + 1 and columns b.x + 2 (ox + x4) .. + 7, inside the same block.  x is a multiple of 4, so the
// 4-byte accesses are aligned.  The shims' kernels index packed blocks by a sample number below w * h.
#include "compound_tile.h"
#include "wedge_masks.h"

static_assert(sizeof(SvtGpuMaskedCompoundBlock) == 32, "SvtGpuMaskedCompoundBlock is 32 bytes");
static_assert(offsetof(SvtGpuMaskedCompoundBlock, filter_y) == offsetof(SvtGpuCompoundBlock, filter_y) &&
                  offsetof(SvtGpuMaskedCompoundBlock, mv1_y) == offsetof(SvtGpuCompoundBlock, mv1_y),
              "the shared fields sit where SvtGpuCompoundBlock has them");

using namespace compound_tile;

namespace {

constexpr int kMaskBase = 38, kDiffFactorLog2 = 4, kMaxAlpha = 64; // DIFFWTD_38's base, DIFF_FACTOR, AOM_BLEND_A64_MAX_ALPHA
enum { kWedge = 0, kDiffWtd = 1 };

// diffwtd_mask_d16's sample: a, b the two CONV_BUF_TYPE values
__device__ __forceinline__ int diffwtd_mask(int a, int b, int inverse, Rounds cr) {
    const int d = a > b ? a - b : b - a;
    const int v = kMaskBase + (round_shift(d, 14 - cr.r0 - cr.r1 + cr.bd - 8) >> kDiffFactorLog2);
    const int m = v > kMaxAlpha ? kMaxAlpha : v;
    return inverse ? kMaxAlpha - m : m;
}
// blend_a64_d16_mask's sample
__device__ __forceinline__ int blend(int m, int s0, int s1, Rounds cr) {
    return compound_finish((m * s0 + (kMaxAlpha - m) * s1) >> 6 /* AOM_BLEND_A64_ROUND_BITS */, cr.r0, cr.r1, cr.bd);
}

// ---------------------------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------------------------
struct MaskedArgs {
    const SvtGpuTfPlanes            *refs;   // [n_refs]
    const SvtGpuMaskedCompoundBlock *blocks; // [n_blocks]
    const CompItem                  *items;  // [n_items] of this launch
    uint8_t                         *mask;   // the state's mask plane (stride width), or null without chroma
    SvtGpuTfPlanes                   pred;
    int32_t                          n_items, width, height, border_x, border_y, bd;
};

template <typename T>
__global__ __launch_bounds__(256) void masked_compound_kernel(const MaskedArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds_all[4 * kWaveLds];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it = blockIdx.x * 4 + wave;
    if (it >= a.n_items) return;
    const CompItem &item = a.items[it];
    const int twl = item.tw_log2, thl = item.th_log2, tw = 1 << twl, th = 1 << thl;
    const int ul = twl + thl - 2, lpl = ul < 6 ? ul : 6, lps = 1 << lpl, slot = lane >> lpl, li = lane & (lps - 1);
    if (slot >= item.nslots) return;
    const CompSlot                  sl = item.slot[slot];
    const SvtGpuMaskedCompoundBlock b  = a.blocks[sl.blk];
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
    const wedge_masks::Plan wp = wedge_masks::plan(b.w_log2, b.h_log2, b.wedge_index, b.wedge_sign); // read for wedge blocks only
    uint8_t *const mrow = a.mask + (size_t)b.y * a.width + b.x; // the block's corner in the mask plane (DIFFWTD with chroma)
    u16x4 conv[2][4]; // the lane's CONV_BUF_TYPE values of both references: at most four units
#pragma unroll
    for (int r = 0; r < 2; r++) {
        ref_pass<T>(a, b, sl, r, px, py, twl, thl, cr, win, im, li, lps,
                     [&](int i, int, int, const int res[4]) __attribute__((always_inline)) {
                         conv[r][i] = (u16x4){(uint16_t)res[0], (uint16_t)res[1], (uint16_t)res[2], (uint16_t)res[3]};
                     });
    }
    // the blend, once per unit and outside the passes' four forms
    const int gl = twl - 2, units = 1 << ul;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = li + i * lps;
        if (u >= units) break;
        const int y = u >> gl, x4 = (u & ((1 << gl) - 1)) << 2;
        const int by = sl.oy + y, bx = sl.ox + x4; // the unit in the block's plane
        int       m[4];
        if (b.comp_type == kWedge) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (!ss) {
                    m[j] = wedge_masks::plan_value(wp, by, bx + j);
                } else {
                    const int yy = 2 * by, xx = 2 * (bx + j);
                    m[j] = (wedge_masks::plan_value(wp, yy, xx) + wedge_masks::plan_value(wp, yy + 1, xx) +
                            wedge_masks::plan_value(wp, yy, xx + 1) + wedge_masks::plan_value(wp, yy + 1, xx + 1) + 2) >> 2;
                }
            }
        } else if (!ss) {
            u8x4 mv;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                m[j]  = diffwtd_mask(conv[0][i][j], conv[1][i][j], b.mask_type, cr);
                mv[j] = (uint8_t)m[j];
            }
            if (a.mask) *(u8x4 *)(mrow + (size_t)by * a.width + bx) = mv;
        } else {
            const uint8_t *q = mrow + (size_t)(2 * by) * a.width + 2 * bx;
            const u8x4     t0 = *(const u8x4 *)q, t1 = *(const u8x4 *)(q + 4);
            const u8x4     u0 = *(const u8x4 *)(q + a.width), u1 = *(const u8x4 *)(q + a.width + 4);
            m[0] = (t0[0] + t0[1] + u0[0] + u0[1] + 2) >> 2, m[1] = (t0[2] + t0[3] + u0[2] + u0[3] + 2) >> 2;
            m[2] = (t1[0] + t1[1] + u1[0] + u1[1] + 2) >> 2, m[3] = (t1[2] + t1[3] + u1[2] + u1[3] + 2) >> 2;
        }
        V4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = (T)blend(m[j], conv[0][i][j], conv[1][i][j], cr);
        *(V4 *)(dst + (size_t)y * pstride + x4) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// the shims' kernels: packed blocks, one lane per sample
// ---------------------------------------------------------------------------------------------
struct MaskArgs {
    const uint16_t *src0, *src1; // packed w x h CONV_BUF_TYPE blocks
    uint8_t        *mask;        // packed w x h
    int32_t         n, inverse;
    Rounds          cr;
};
__global__ __launch_bounds__(256) void diffwtd_mask_kernel(const MaskArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) a.mask[i] = (uint8_t)diffwtd_mask(a.src0[i], a.src1[i], a.inverse, a.cr);
}

struct BlendArgs {
    const uint16_t *src0, *src1; // packed w x h CONV_BUF_TYPE blocks
    const uint8_t  *mask;        // packed (w << subw) x (h << subh)
    void           *dst;         // packed w x h
    int32_t         w_log2, n, subw, subh;
    Rounds          cr;
};
template <typename T>
__global__ __launch_bounds__(256) void blend_d16_kernel(const BlendArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int      y = i >> a.w_log2, x = i & ((1 << a.w_log2) - 1), ms = 1 << (a.w_log2 + a.subw);
    const uint8_t *q = a.mask + (size_t)(y << a.subh) * ms + (x << a.subw);
    int            m;
    if (a.subw && a.subh)
        m = (q[0] + q[ms] + q[1] + q[ms + 1] + 2) >> 2;
    else if (a.subw)
        m = (q[0] + q[1] + 1) >> 1; // AOM_BLEND_AVG
    else if (a.subh)
        m = (q[0] + q[ms] + 1) >> 1;
    else
        m = q[0];
    ((T *)a.dst)[i] = (T)blend(m, a.src0[i], a.src1[i], a.cr);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
void shim_mask(uint8_t *mask, int mask_type, const uint16_t *src0, int src0_stride, const uint16_t *src1, int src1_stride, int h,
               int w, int round_0, int round_1, int bd) {
    if (!mask || !src0 || !src1 || !size_ok(w, 4) || !size_ok(h, 4) || src0_stride < w || src1_stride < w || mask_type < 0 ||
        mask_type > 1 || (bd != 8 && bd != 10 && bd != 12) || !rounds_ok(round_0, round_1))
        svtgpu_fatal("svtgpu diffwtd mask shim: bad arguments");
    const size_t  blk = (size_t)w * h * 2;
    Carver        c; // src0 at 0, src1, the mask
    c(blk);
    const size_t  o1 = c(blk), om = c((size_t)w * h);
    hipStream_t   st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t *const hb = sg.h, *const d = sg.d;
    pack_rows(hb, src0, (size_t)src0_stride * 2, (size_t)w * 2, h);
    pack_rows(hb + o1, src1, (size_t)src1_stride * 2, (size_t)w * 2, h);
    HIP_OR_DIE(hipMemcpyAsync(d, hb, om, hipMemcpyHostToDevice, st));
    MaskArgs a;
    memset(&a, 0, sizeof a);
    a.src0 = (const uint16_t *)d, a.src1 = (const uint16_t *)(d + o1), a.mask = d + om, a.n = w * h, a.inverse = mask_type;
    a.cr = {round_0, round_1, bd};
    hipLaunchKernelGGL(diffwtd_mask_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(hb + om, d + om, (size_t)w * h, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    memcpy(mask, hb + om, (size_t)w * h); // the reference packs the mask with stride w
}

template <typename T>
void shim_blend(T *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride, const uint16_t *src1, uint32_t src1_stride,
                const uint8_t *mask, uint32_t mask_stride, int w, int h, int subw, int subh, int round_0, int round_1, int bd) {
    if (!dst || !src0 || !src1 || !mask || !size_ok(w, 4) || !size_ok(h, 4) || subw < 0 || subw > 1 || subh < 0 || subh > 1 ||
        dst_stride < (uint32_t)w || src0_stride < (uint32_t)w || src1_stride < (uint32_t)w || mask_stride < (uint32_t)(w << subw) ||
        (sizeof(T) == 1 ? bd != 8 : (bd != 8 && bd != 10 && bd != 12)) || !rounds_ok(round_0, round_1))
        svtgpu_fatal("svtgpu blend_a64_d16_mask shim: bad arguments");
    const int    mw = w << subw, mh = h << subh;
    const size_t blk = (size_t)w * h * 2, out = (size_t)w * h * sizeof(T);
    Carver       c; // src0 at 0, src1, the mask, the pixels
    c(blk);
    const size_t o1 = c(blk), om = c((size_t)mw * mh), oo = c(out);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t *const hb = sg.h, *const d = sg.d;
    // src0 / src1 may be dst itself in the reference's contract: everything is read before anything is written
    pack_rows(hb, src0, (size_t)src0_stride * 2, (size_t)w * 2, h);
    pack_rows(hb + o1, src1, (size_t)src1_stride * 2, (size_t)w * 2, h);
    pack_rows(hb + om, mask, mask_stride, (size_t)mw, mh);
    HIP_OR_DIE(hipMemcpyAsync(d, hb, oo, hipMemcpyHostToDevice, st));
    BlendArgs a;
    memset(&a, 0, sizeof a);
    a.src0 = (const uint16_t *)d, a.src1 = (const uint16_t *)(d + o1), a.mask = d + om, a.dst = d + oo;
    a.w_log2 = log2_of(w), a.n = w * h, a.subw = subw, a.subh = subh, a.cr = {round_0, round_1, bd};
    hipLaunchKernelGGL(blend_d16_kernel<T>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(hb + oo, d + oo, out, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    unpack_rows(dst, (ptrdiff_t)dst_stride * sizeof(T), hb + oo, (size_t)w * sizeof(T), h);
}

} // namespace

extern "C" int svtgpu_wedge_mask(int32_t w, int32_t h, int32_t wedge_index, int32_t wedge_sign, uint8_t *mask) {
    if (!mask || w < 8 || h < 8 || w > 32 || h > 32 || (w & (w - 1)) || (h & (h - 1)) || wedge_index < 0 ||
        wedge_index >= wedge_masks::kIndices || wedge_sign < 0 || wedge_sign > 1)
        return SVTGPU_ERR_INVALID_ARG;
    const int wl = log2_of(w), hl = log2_of(h);
    if (!wedge_masks::bits(wl, hl)) return SVTGPU_ERR_INVALID_ARG;
    wedge_masks::fill(wl, hl, wedge_index, wedge_sign, mask);
    return SVTGPU_OK;
}

extern "C" int svtgpu_masked_compound_predict_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                                    int32_t border_y, const SvtGpuMaskedCompoundBlock *blocks, int32_t n_blocks,
                                                    int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream) {
    auto block_ok = [](const SvtGpuMaskedCompoundBlock &b) {
        for (uint8_t v : b.reserved)
            if (v) return false;
        return b.comp_type <= 1 && b.wedge_index < wedge_masks::kIndices && b.wedge_sign <= 1 && b.mask_type <= 1 &&
               (b.comp_type != kWedge || wedge_masks::bits(b.w_log2, b.h_log2));
    };
    // the DIFFWTD chroma tiles read the masks that the luma tiles of the first launch write
    return tile_batch<MaskedArgs>(
        s, refs, n_refs, border_x, border_y, blocks, n_blocks, bit_depth, chroma, pred, stream, masked_compound_kernel<uint8_t>,
        masked_compound_kernel<uint16_t>, block_ok, [](const SvtGpuMaskedCompoundBlock &b) { return b.comp_type == kDiffWtd; },
        [&](MaskedArgs &a, bool has_later) { return has_later ? svtgpu_tf_mask_reserve(s, &a.mask) : 0; });
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous.  svtgpu_rtcd.h's adapters spell the reference's ConvolveParams out.
// ---------------------------------------------------------------------------------------------
extern "C" void svtgpu_av1_build_compound_diffwtd_mask_d16(uint8_t *mask, int32_t mask_type, const uint16_t *src0,
                                                           int32_t src0_stride, const uint16_t *src1, int32_t src1_stride, int32_t h,
                                                           int32_t w, int32_t round_0, int32_t round_1, int32_t bd) {
    shim_mask(mask, mask_type, src0, src0_stride, src1, src1_stride, h, w, round_0, round_1, bd);
}
extern "C" void svtgpu_aom_lowbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                                    const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask,
                                                    uint32_t mask_stride, int32_t w, int32_t h, int32_t subw, int32_t subh,
                                                    int32_t round_0, int32_t round_1) {
    shim_blend<uint8_t>(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subw, subh, round_0, round_1, 8);
}
extern "C" void svtgpu_aom_highbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                                     const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask,
                                                     uint32_t mask_stride, int32_t w, int32_t h, int32_t subw, int32_t subh,
                                                     int32_t round_0, int32_t round_1, int32_t bd) {
    // the reference's dst is a uint8_t * it casts to uint16_t * (EbBlend_a64_mask.c:113)
    shim_blend<uint16_t>((uint16_t *)dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subw, subh, round_0,
                         round_1, bd);
}
