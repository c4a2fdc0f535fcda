// masked_compound.hip — AV1 masked compound prediction on gfx950: COMPOUND_WEDGE and COMPOUND_DIFFWTD, the other two of
// the four inter-inter compound types.  svt_av1_build_compound_diffwtd_mask_d16_c (C_DEFAULT/EbInterPrediction_c.c:15-40),
// svt_aom_lowbd_blend_a64_d16_mask_c / svt_aom_highbd_blend_a64_d16_mask_c (EbBlend_a64_mask.c:34-195) behind three RTCD
// shims, the wedge masks of svt_av1_init_wedge_masks (csrc/wedge_masks.h), and the masked bi-predicted blocks of a picture
// (svt_aom_inter_prediction with a masked compound type: reference 1 through av1_make_masked_scaled_inter_predictor,
// EbEncInterPrediction.c:50-164) as svtgpu_masked_compound_predict_batch.
//
// The two reference passes of a tile are compound.hip's (csrc/compound_tile.h): reference 0's CONV_BUF_TYPE values stay
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
    const int offset_bits = cr.bd + 14 - cr.r0, top = (1 << cr.bd) - 1;
    int       res = (m * s0 + (kMaxAlpha - m) * s1) >> 6; // AOM_BLEND_A64_ROUND_BITS
    res -= (1 << (offset_bits - cr.r1)) + (1 << (offset_bits - cr.r1 - 1));
    const int v = round_shift(res, 14 - cr.r0 - cr.r1);
    return v < 0 ? 0 : v > top ? top : v;
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

    const int    p = sl.plane, ss = p > 0, sc = 1 - ss;
    const int    bw = 1 << b.w_log2, bh = 1 << b.h_log2, pbw = bw >> ss, pbh = bh >> ss; // the block in luma and in the plane
    const int    pw = a.width >> ss, ph = a.height >> ss, bdx = a.border_x >> ss, bdy = a.border_y >> ss;
    // the block's origin in the plane: chroma at ((x >> 3) << 3) / 2 (EbEncInterPrediction.c:4269)
    const int    px = ss ? ((b.x >> 3) << 3) >> 1 : b.x, py = ss ? ((b.y >> 3) << 3) >> 1 : b.y;
    const Rounds cr = {3, 7, a.bd}; // get_conv_params_no_round(is_compound = 1) at 8 and 10 bits
    const int    fxt = filter_table(b.filter_x, pbw), fyt = filter_table(b.filter_y, pbh);
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
        const SvtGpuTfPlanes &rp = a.refs[r ? b.ref1 : b.ref0];
        // clamp_mv_to_umv_border_sb (:28-48) with the block's own edges, 1/16 sample of the plane
        int       qx = (int16_t)((r ? b.mv1_x : b.mv0_x) * (1 << sc)), qy = (int16_t)((r ? b.mv1_y : b.mv0_y) * (1 << sc));
        const int spx = (4 + pbw) << 4, spy = (4 + pbh) << 4;
        const int lo_x = -(b.x * 8) * (1 << sc) - spx, hi_x = ((a.width - bw - b.x) * 8) * (1 << sc) + spx - 16;
        const int lo_y = -(b.y * 8) * (1 << sc) - spy, hi_y = ((a.height - bh - b.y) * 8) * (1 << sc) + spy - 16;
        qx = (int16_t)clamp_i(qx, lo_x, hi_x), qy = (int16_t)clamp_i(qy, lo_y, hi_y);
        const int phx = qx & 15, phy = qy & 15, mode = (phx ? kHorz : 0) | (phy ? kVert : 0);
        const int sx = px + (qx >> 4) + sl.ox, sy = py + (qy >> 4) + sl.oy;
        tile_pass<T>((const T *)rp.plane[p], rp.stride[p], -bdx, pw + bdx - 1, -bdy, ph + bdy - 1, sx, sy, twl, thl, mode,
                     kInterpFilters[fxt][phx], kInterpFilters[fyt][phy], cr, win, im, li, lps,
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
bool rounds_ok(int r0, int r1) { return r0 >= 0 && r0 <= 7 && r1 >= 0 && r1 <= 7 && 14 - r0 - r1 >= 0; }
int  log2_of(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}
void pack_rows(uint8_t *to, const void *from, size_t from_stride_bytes, size_t row_bytes, int rows) {
    for (int y = 0; y < rows; y++) memcpy(to + (size_t)y * row_bytes, (const uint8_t *)from + (size_t)y * from_stride_bytes, row_bytes);
}

void shim_mask(uint8_t *mask, int mask_type, const uint16_t *src0, int src0_stride, const uint16_t *src1, int src1_stride, int h,
               int w, int round_0, int round_1, int bd) {
    if (!mask || !src0 || !src1 || !size_ok(w) || !size_ok(h) || src0_stride < w || src1_stride < w || mask_type < 0 ||
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
    if (!dst || !src0 || !src1 || !mask || !size_ok(w) || !size_ok(h) || subw < 0 || subw > 1 || subh < 0 || subh > 1 ||
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
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * dst_stride, hb + oo + (size_t)y * w * sizeof(T), (size_t)w * sizeof(T));
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
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!s || !refs || !pred || n_refs < 0 || n_blocks < 0 || (n_blocks && !blocks) || (bit_depth != 8 && bit_depth != 10) ||
        border_x < 0 || border_y < 0)
        return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    const int bs = bit_depth > 8 ? 2 : 1, nplanes = chroma ? 3 : 1; // without chroma planes 1 and 2 are not looked at
    for (int p = 0; p < nplanes; p++) {
        const int ss = p > 0;
        for (int r = 0; r < n_refs; r++)
            if (!refs[r].plane[p] || ((uintptr_t)refs[r].plane[p] & (bs - 1)) ||
                refs[r].stride[p] < (width >> ss) + 2 * (border_x >> ss))
                return SVTGPU_ERR_INVALID_ARG;
        if (!pred->plane[p] || pred->stride[p] < (width >> ss) || (((size_t)pred->stride[p] * bs) & 15) ||
            ((uintptr_t)pred->plane[p] & 15))
            return SVTGPU_ERR_INVALID_ARG;
    }
    // first: every wedge tile and the DIFFWTD luma tiles; second: the DIFFWTD chroma tiles, which read the first's masks
    ItemBuilder first, second;
    for (int i = 0; i < n_blocks; i++) {
        const SvtGpuMaskedCompoundBlock &b = blocks[i];
        if (!block_size_ok(b.w_log2, b.h_log2) || b.x < 0 || b.y < 0 || (b.x & 3) || (b.y & 3) ||
            b.x + (1 << b.w_log2) > width || b.y + (1 << b.h_log2) > height || b.ref0 >= n_refs || b.ref1 >= n_refs ||
            b.filter_x > 3 || b.filter_y > 3 || b.comp_type > 1 || b.wedge_index >= wedge_masks::kIndices || b.wedge_sign > 1 ||
            b.mask_type > 1 || (b.comp_type == kWedge && !wedge_masks::bits(b.w_log2, b.h_log2)))
            return SVTGPU_ERR_INVALID_ARG;
        for (uint8_t v : b.reserved)
            if (v) return SVTGPU_ERR_INVALID_ARG;
        for (int p = 0; p < nplanes; p++) (p && b.comp_type == kDiffWtd ? second : first).add_plane((uint32_t)i, p, b.w_log2, b.h_log2);
    }
    if (!n_blocks) return SVTGPU_OK;
    uint8_t *mask = nullptr;
    if (!second.items.empty())
        if (int rc = svtgpu_tf_mask_reserve(s, &mask)) return rc;
    hipStream_t  st = pick_stream(ctx, stream);
    const size_t n1 = first.items.size(), n2 = second.items.size();
    const size_t o_blk = align16((size_t)n_refs * sizeof(SvtGpuTfPlanes)), o_item = o_blk + (size_t)n_blocks * sizeof(SvtGpuMaskedCompoundBlock);
    const size_t total = o_item + (n1 + n2) * sizeof(CompItem);
    uint8_t     *hm, *dm;
    if (int rc = svtgpu_tf_meta_begin(s, total, &hm, &dm)) return rc;
    memcpy(hm, refs, (size_t)n_refs * sizeof(SvtGpuTfPlanes));
    memcpy(hm + o_blk, blocks, (size_t)n_blocks * sizeof(SvtGpuMaskedCompoundBlock));
    memcpy(hm + o_item, first.items.data(), n1 * sizeof(CompItem));
    if (n2) memcpy(hm + o_item + n1 * sizeof(CompItem), second.items.data(), n2 * sizeof(CompItem));
    if (int rc = svtgpu_tf_meta_upload(s, total, st)) return rc;
    MaskedArgs a;
    memset(&a, 0, sizeof a);
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const SvtGpuMaskedCompoundBlock *)(dm + o_blk), a.mask = mask, a.pred = *pred;
    a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y, a.bd = bit_depth;
    const CompItem *d_items = (const CompItem *)(dm + o_item);
    for (int pass = 0; pass < 2; pass++) {
        const size_t n = pass ? n2 : n1;
        if (!n) continue;
        a.items = d_items + (pass ? n1 : 0), a.n_items = (int32_t)n;
        const dim3 grid((unsigned)((n + 3) / 4));
        if (bit_depth == 8)
            hipLaunchKernelGGL(masked_compound_kernel<uint8_t>, grid, dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(masked_compound_kernel<uint16_t>, grid, dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return SVTGPU_OK;
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
