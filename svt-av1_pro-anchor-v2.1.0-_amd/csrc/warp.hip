// warp.hip — AV1 warped-motion (affine) inter prediction on gfx950: svt_av1_warp_affine_c / svt_av1_highbd_warp_affine_c
// (EbWarpedMotion.c:570, :822) behind two RTCD shims, and the warped blocks of a picture (svt_aom_warped_motion_prediction,
// EbEncInterPrediction.c:2747, through plane_warped_motion_prediction, :2051, with no masked compound) as one launch,
// svtgpu_warp_predict_batch.  The tables and the shear parameters are csrc/warp_params.h; the item list and the entry's
// checks are csrc/pred_plan.h.
//
//   unit         the 8x8 outputs of one plane of one block that share a projected origin: the work of one wave, lane
//                (k, l) = (lane / 8, lane % 8) owning output row k, column l.  The origin (ix4, iy4) and the two fractional
//                starts (sx4, sy4) are the same for the whole wave and live in scalar registers.
//   patch        the wave stages the 15 x 15 source samples rows iy4 - 7 .. + 7, columns ix4 - 7 .. + 7 into LDS once, each
//                coordinate clamped to the plane at staging (the C clamps every read; nothing outside the visible picture is
//                read).  Row stride 16 samples, so a lane's 8 consecutive samples are five aligned 32-bit reads.
//   horizontal   15 rows x 8 columns = 120 results, two per lane (the second for rows 8 .. 14), each with its own row of the
//                warped filter table: sx = sx4 + beta * (row - 3) + alpha * l.  The results go to LDS as 16-bit values: they
//                fit (bd + 8 - reduce_bits_horiz bits: 13 at 8 bits, 15 at 10 and 12).
//   vertical     per lane from there, filter row by sy = sy4 + delta * k + gamma * l.
//   compound     both references of a block in the same wave, one after the other; the first one's CONV_BUF_TYPE value stays
//                in the lane's register.  No intermediate reaches global memory.
//   table        193 rows x 16 bytes = 3088 bytes of LDS per workgroup, loaded once; a lane fetches its row with one
//                128-bit LDS read.
//   workgroup    four waves = four units, given by one item of the host's list: up to 2 x 2 units of a plane's block (1 x 4
//                for an 8-wide one).  An item never spans blocks or planes, so a plane's block of fewer than four units (8x8 and
//                8x16 luma, the chroma of 16x16 and 16x32) leaves waves of its workgroup idle, and still loads the table.  One workgroup barrier, after the table load and before any wave leaves; from there a
//                wave's LDS slice is private and its DS operations complete in order.
//
// Bounds.  Reference reads: row and column clamped into [0, height - 1] x [0, width - 1] of the plane (chroma: halved), which
// the entry checked the strides against.  Predictor writes: inside the block, which the entry checked against the state's
// picture area.  blocks[] / refs[] indices are checked on the host.  The shims' kernel reads the staged rectangle that the
// host computed with the same integer arithmetic from every unit's clamped rows and columns, and indexes the packed
// p_width x p_height blocks by a position inside them.
#include "compound_tile.h"
#include "compound_weights.h"
#include "warp_params.h"

static_assert(sizeof(SvtGpuWarpBlock) == 64, "SvtGpuWarpBlock is 64 bytes");
static_assert(offsetof(SvtGpuWarpBlock, wmmat0) == 12 && offsetof(SvtGpuWarpBlock, wmmat1) == 36, "the models sit behind 12 bytes");

using namespace conv_device;
using namespace pred_plan;

namespace {

namespace wp = warp_params;

constexpr int kPatchStride = 16, kPatchRows = 15;
constexpr int kWaveWork    = kPatchRows * kPatchStride + kPatchRows * 8; // 16-bit elements per wave: patch, then intermediate
constexpr int kNoRef       = 0xFF;

struct Model { // one reference's model as the kernels take it
    int32_t mat[6];
    int16_t abgd[4];
};
struct Shifts { // the C functions' derived constants
    int32_t bd, rbh, r0, r1; // bit depth, reduce_bits_horiz, ConvolveParams::round_0 / round_1
};

// The workgroup's copy of the filter table.  Every thread of the workgroup calls it.
__device__ __forceinline__ void load_table(int16_t *tab) {
    if (threadIdx.x < wp::kFilterRows) ((uint4 *)tab)[threadIdx.x] = ((const uint4 *)wp::kFilter.row)[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ int dot8(const uint32_t p[4], const int16_t *coeffs) {
    const compound_tile::i16x8 c = *(const compound_tile::i16x8 *)coeffs;
    int                        s = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) s += (int)(p[m] & 0xffff) * c[2 * m] + (int)(p[m] >> 16) * c[2 * m + 1];
    return s;
}

// One unit of one reference: the vertical filter's sum of the lane's output (the 1 << offset_bits_vert included, before
// any rounding).  (j, i) is the unit's top-left in the plane; `ref` points at sample (0, 0) of the plane minus (x0, y0)
// samples (the batch: x0 = y0 = 0).
template <typename T>
__device__ __forceinline__ int warp_unit(const T *__restrict__ ref, int stride, int width, int height, const Model &m, int ssx, int ssy,
                                         int j, int i, const Shifts sh, const int16_t *tab, uint16_t *patch, uint16_t *im, int lane) {
    const int alpha = m.abgd[0], beta = m.abgd[1], gamma = m.abgd[2], delta = m.abgd[3];
    const int src_x = (j + 4) << ssx, src_y = (i + 4) << ssy;
    // the host has checked that neither sum leaves int32
    const int dst_x = m.mat[2] * src_x + m.mat[3] * src_y + m.mat[0], dst_y = m.mat[4] * src_x + m.mat[5] * src_y + m.mat[1];
    const int x4 = dst_x >> ssx, y4 = dst_y >> ssy;
    const int ix4 = x4 >> wp::kModelPrecBits, iy4 = y4 >> wp::kModelPrecBits;
    const int frac = (1 << wp::kModelPrecBits) - 1, keep = ~((1 << wp::kReduceBits) - 1);
    const int sx4 = ((x4 & frac) + alpha * -4 + beta * -4) & keep, sy4 = ((y4 & frac) + gamma * -4 + delta * -4) & keep;

    wave_lds_sync(); // the previous reference's reads of patch and im are done
    { // sixteen lanes to a patch row (the sixteenth idle), four rows at a time: no division, one column clamp per lane
        const int c = lane & 15, gx = clamp_i(ix4 - 7 + c, 0, width - 1);
#pragma unroll
        for (int r = lane >> 4; r < kPatchRows; r += 4) {
            const int gy = clamp_i(iy4 - 7 + r, 0, height - 1);
            if (c < kPatchRows) patch[r * kPatchStride + c] = ref[(ptrdiff_t)gy * stride + gx];
        }
    }
    wave_lds_sync();
    const int k = lane >> 3, l = lane & 7;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int r = k + 8 * half; // intermediate row 0 .. 14: the C's k = r - 7
        if (r < kPatchRows) {
            const int       sx   = sx4 + beta * (r - 3) + alpha * l;
            const int       offs = round_shift(sx, wp::kDiffPrecBits) + wp::kPixelShifts;
            const uint32_t *q    = (const uint32_t *)(patch + r * kPatchStride) + (l >> 1);
            const uint32_t  w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            const uint32_t  s = (l & 1) * 16;
            const uint32_t  p[4] = {__builtin_amdgcn_alignbit(w1, w0, s), __builtin_amdgcn_alignbit(w2, w1, s),
                                    __builtin_amdgcn_alignbit(w3, w2, s), __builtin_amdgcn_alignbit(w4, w3, s)};
            const int       sum  = (1 << (sh.bd + 6)) + dot8(p, tab + 8 * offs);
            im[r * 8 + l] = (uint16_t)round_shift(sum, sh.rbh);
        }
    }
    wave_lds_sync();
    const int sy = sy4 + delta * k + gamma * l, offs = round_shift(sy, wp::kDiffPrecBits) + wp::kPixelShifts;
    const compound_tile::i16x8 c = *(const compound_tile::i16x8 *)(tab + 8 * offs);
    int                        sum = 1 << (sh.bd + 14 - sh.rbh);
#pragma unroll
    for (int t = 0; t < 8; t++) sum += (int)im[(k + t) * 8 + l] * c[t];
    return sum;
}

// how a sum becomes a value without a second reference (the tail of the C's vertical loop; with one: compound_average)
__device__ __forceinline__ int single_pixel(int sum, const Shifts sh) { // not compound
    const int top = (1 << sh.bd) - 1, v = round_shift(sum, 14 - sh.rbh) - (1 << (sh.bd - 1)) - (1 << sh.bd);
    return v < 0 ? 0 : v > top ? top : v;
}

// ---------------------------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------------------------
struct DevBlock { // what the kernel needs of a SvtGpuWarpBlock, with the host's shear parameters; 76 bytes
    int16_t x, y;
    uint8_t w_log2, h_log2, ref0, ref1, dist_wtd, fwd_offset, bck_offset, pad;
    Model   m[2];
};
static_assert(sizeof(DevBlock) == 76, "DevBlock is 76 bytes");
struct WarpArgs {
    const SvtGpuTfPlanes *refs;   // [n_refs]
    const DevBlock       *blocks; // [n_blocks]
    const WarpItem       *items;  // [gridDim.x]
    SvtGpuTfPlanes        pred;
    int32_t               width, height, bd;
};

template <typename T>
__global__ __launch_bounds__(256) void warp_kernel(const WarpArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t  tab[wp::kFilterRows * 8];
    __shared__ __attribute__((aligned(16))) uint16_t work[4 * kWaveWork];
    load_table(tab);
    const int      lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const WarpItem it = a.items[blockIdx.x];
    int            gw, n;
    warp_shape_decode(it.shape, &gw, &n);
    if (wave >= n) return;
    const DevBlock &b = a.blocks[it.blk];
    const int       p = it.plane, ss = p > 0;
    const int       ux = it.ux + (gw == 2 ? (wave & 1) : 0), uy = it.uy + (gw == 2 ? (wave >> 1) : wave);
    const int       px = b.x >> ss, py = b.y >> ss, pw = a.width >> ss, ph = a.height >> ss; // b.x, b.y are multiples of 8
    const int       j = px + 8 * ux, i = py + 8 * uy;
    uint16_t       *patch = work + wave * kWaveWork, *im = patch + kPatchRows * kPatchStride;
    const bool      two = b.ref1 != kNoRef;
    const Shifts    sh = {a.bd, 3, 3, two ? 7 : 11}; // get_conv_params_no_round at 8 and 10 bits; reduce_bits_horiz = round_0 there
    // the plane by selects, not by a lane-varying index into the kernel arguments
    void *const pplane  = p == 0 ? a.pred.plane[0] : p == 1 ? a.pred.plane[1] : a.pred.plane[2];
    const int   pstride = p == 0 ? a.pred.stride[0] : p == 1 ? a.pred.stride[1] : a.pred.stride[2];
    T          *dst = (T *)pplane + (size_t)(i + (lane >> 3)) * pstride + j + (lane & 7);
    const SvtGpuTfPlanes &r0 = a.refs[b.ref0];
    const int sum0 = warp_unit<T>((const T *)(p == 0 ? r0.plane[0] : p == 1 ? r0.plane[1] : r0.plane[2]),
                                  p == 0 ? r0.stride[0] : p == 1 ? r0.stride[1] : r0.stride[2], pw, ph, b.m[0], ss, ss, j, i, sh, tab,
                                  patch, im, lane);
    if (!two) {
        *dst = (T)single_pixel(sum0, sh);
        return;
    }
    const int             first = round_shift(sum0, sh.r1); // the CONV_BUF_TYPE value
    const SvtGpuTfPlanes &r1 = a.refs[b.ref1];
    const int sum1 = warp_unit<T>((const T *)(p == 0 ? r1.plane[0] : p == 1 ? r1.plane[1] : r1.plane[2]),
                                  p == 0 ? r1.stride[0] : p == 1 ? r1.stride[1] : r1.stride[2], pw, ph, b.m[1], ss, ss, j, i, sh, tab,
                                  patch, im, lane);
    *dst = (T)compound_average(first, round_shift(sum1, sh.r1), b.dist_wtd, b.fwd_offset, b.bck_offset, sh.r0, sh.r1,
                               sh.bd);
}

// ---------------------------------------------------------------------------------------------
// the shims' kernel: `ref` is the staged rectangle [x0, x1] x [y0, y1] of the plane (stride x1 - x0 + 1); conv the packed
// p_width x p_height CONV_BUF_TYPE block (written on a first pass, read on a second); dst the packed pixel block.
// ---------------------------------------------------------------------------------------------
struct ShimArgs {
    const void *ref;
    uint16_t   *conv;
    void       *dst;
    Model       m;
    Shifts      sh;
    int32_t     x0, y0, stride, width, height, p_col, p_row, p_width, p_height, ssx, ssy;
    int32_t     is_compound, do_average, dist_wtd, fwd, bck;
};
template <typename T>
__global__ __launch_bounds__(256) void warp_block_kernel(const ShimArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t  tab[wp::kFilterRows * 8];
    __shared__ __attribute__((aligned(16))) uint16_t work[4 * kWaveWork];
    load_table(tab);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int uw = a.p_width >> 3, u = blockIdx.x * 4 + wave;
    if (u >= uw * (a.p_height >> 3)) return;
    const int uy = u / uw, ux = u - uy * uw;
    uint16_t *patch = work + wave * kWaveWork, *im = patch + kPatchRows * kPatchStride;
    const T  *ref = (const T *)a.ref - ((ptrdiff_t)a.y0 * a.stride + a.x0);
    const int sum = warp_unit<T>(ref, a.stride, a.width, a.height, a.m, a.ssx, a.ssy, a.p_col + 8 * ux, a.p_row + 8 * uy, a.sh, tab,
                                 patch, im, lane);
    const size_t at = (size_t)(8 * uy + (lane >> 3)) * a.p_width + 8 * ux + (lane & 7);
    if (!a.is_compound)
        ((T *)a.dst)[at] = (T)single_pixel(sum, a.sh);
    else if (!a.do_average)
        a.conv[at] = (uint16_t)round_shift(sum, a.sh.r1);
    else
        ((T *)a.dst)[at] = (T)compound_average(a.conv[at], round_shift(sum, a.sh.r1), a.dist_wtd, a.fwd, a.bck, a.sh.r0, a.sh.r1,
                                               a.sh.bd);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// the projection of the unit at (j, i) of a plane in 64 bits: false when either sum leaves int32 (the C is undefined there)
bool project(const int32_t *mat, int ssx, int ssy, int j, int i, int64_t *dst_x, int64_t *dst_y) {
    const int64_t src_x = (int64_t)(j + 4) << ssx, src_y = (int64_t)(i + 4) << ssy;
    *dst_x = (int64_t)mat[2] * src_x + (int64_t)mat[3] * src_y + mat[0];
    *dst_y = (int64_t)mat[4] * src_x + (int64_t)mat[5] * src_y + mat[1];
    // the partial sums too: the C adds left to right
    const int64_t px = (int64_t)mat[2] * src_x, py = (int64_t)mat[4] * src_x, qx = px + (int64_t)mat[3] * src_y, qy = py + (int64_t)mat[5] * src_y;
    for (int64_t v : {px, py, (int64_t)mat[3] * src_y, (int64_t)mat[5] * src_y, qx, qy, *dst_x, *dst_y})
        if (v < INT32_MIN || v > INT32_MAX) return false;
    return true;
}

// One shim call.  ref8 / ref2: the 8-bit plane and, for the split highbd layout, the plane of the two low bits.
template <typename T>
int shim_warp(const int32_t *mat, const uint8_t *ref8, const uint8_t *ref2, int width, int height, int stride8, int stride2, T *pred,
              int p_col, int p_row, int p_width, int p_height, int p_stride, int ssx, int ssy, int bd, int round_0, int round_1,
              int is_compound, uint16_t *conv_dst, int conv_dst_stride, int do_average, int use_jnt_comp_avg, int fwd_offset,
              int bck_offset, int alpha, int beta, int gamma, int delta) {
    const bool hbd = sizeof(T) == 2;
    const bool writes_pred = !is_compound || do_average;
    if (!mat || !ref8 || (hbd && !ref2) || width < 1 || height < 1 || stride8 < width || (hbd && stride2 < width) || p_col < 0 ||
        p_row < 0 || p_width < 8 || p_height < 8 || (p_width & 7) || (p_height & 7) || p_width > 128 || p_height > 128 || ssx < 0 ||
        ssx > 1 || ssy < 0 || ssy > 1 || (hbd ? (bd != 10 && bd != 12) : bd != 8) || round_0 < 0 || round_0 > 7 ||
        (writes_pred && (!pred || p_stride < p_width)) || (do_average && !is_compound) ||
        (is_compound && (!conv_dst || conv_dst_stride < p_width || round_1 < 0 || round_1 > 7 || 14 - round_0 - round_1 < 0)) ||
        !wp::shear_allowed(alpha, beta, gamma, delta))
        return SVTGPU_ERR_INVALID_ARG;
    const int rbh = hbd ? round_0 + (bd + 7 - round_0 - 14 > 0 ? bd + 7 - round_0 - 14 : 0) : round_0;
    if (bd + 8 - rbh > 16 || 14 - rbh < 0) return SVTGPU_ERR_INVALID_ARG; // the intermediate is kept in 16 bits
    // the rectangle of the plane the units read, with the C's own arithmetic
    int x0 = width, x1 = -1, y0 = height, y1 = -1;
    for (int i = p_row; i < p_row + p_height; i += 8)
        for (int j = p_col; j < p_col + p_width; j += 8) {
            int64_t dx, dy;
            if (!project(mat, ssx, ssy, j, i, &dx, &dy)) return SVTGPU_ERR_INVALID_ARG;
            const int ix4 = (int)((dx >> ssx) >> wp::kModelPrecBits), iy4 = (int)((dy >> ssy) >> wp::kModelPrecBits);
            auto      cl = [](int64_t v, int hi) { return (int)(v < 0 ? 0 : v > hi ? hi : v); };
            const int a0 = cl((int64_t)ix4 - 7, width - 1), a1 = cl((int64_t)ix4 + 7, width - 1);
            const int b0 = cl((int64_t)iy4 - 7, height - 1), b1 = cl((int64_t)iy4 + 7, height - 1);
            x0 = a0 < x0 ? a0 : x0, x1 = a1 > x1 ? a1 : x1, y0 = b0 < y0 ? b0 : y0, y1 = b1 > y1 ? b1 : y1;
        }
    const int    sw = x1 - x0 + 1, shh = y1 - y0 + 1;
    const size_t win = (size_t)sw * shh * sizeof(T), conv = (size_t)p_width * p_height * 2, out = (size_t)p_width * p_height * sizeof(T);
    Carver       c; // the rectangle at 0, then conv_dst and the pixels
    c(win);
    const size_t o_conv = c(conv), o_out = c(out);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t *const hb = sg.h, *const d = sg.d;
    for (int y = 0; y < shh; y++) {
        const uint8_t *s8 = ref8 + (ptrdiff_t)(y0 + y) * stride8 + x0;
        T             *to = (T *)hb + (size_t)y * sw;
        if (!hbd) {
            memcpy(to, s8, (size_t)sw);
        } else {
            const uint8_t *s2 = ref2 + (ptrdiff_t)(y0 + y) * stride2 + x0;
            for (int x = 0; x < sw; x++) to[x] = (T)((s8[x] << 2) | ((s2[x] >> 6) & 3));
        }
    }
    size_t up = win;
    if (is_compound && do_average) {
        pack_rows(hb + o_conv, conv_dst, (ptrdiff_t)conv_dst_stride * 2, (size_t)p_width * 2, p_height);
        up = o_conv + conv;
    }
    HIP_OR_DIE(hipMemcpyAsync(d, hb, up, hipMemcpyHostToDevice, st));
    ShimArgs a;
    memset(&a, 0, sizeof a);
    a.ref = d, a.conv = (uint16_t *)(d + o_conv), a.dst = d + o_out;
    memcpy(a.m.mat, mat, sizeof a.m.mat);
    a.m.abgd[0] = (int16_t)alpha, a.m.abgd[1] = (int16_t)beta, a.m.abgd[2] = (int16_t)gamma, a.m.abgd[3] = (int16_t)delta;
    a.sh = {bd, rbh, round_0, is_compound ? round_1 : 14 - rbh};
    a.x0 = x0, a.y0 = y0, a.stride = sw, a.width = width, a.height = height, a.p_col = p_col, a.p_row = p_row, a.p_width = p_width,
    a.p_height = p_height, a.ssx = ssx, a.ssy = ssy, a.is_compound = is_compound, a.do_average = do_average,
    a.dist_wtd = use_jnt_comp_avg, a.fwd = fwd_offset, a.bck = bck_offset;
    const int units = (p_width >> 3) * (p_height >> 3);
    hipLaunchKernelGGL(warp_block_kernel<T>, dim3((unsigned)((units + 3) / 4)), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    const size_t o_back = writes_pred ? o_out : o_conv, n_back = writes_pred ? out : conv;
    HIP_OR_DIE(hipMemcpyAsync(hb + o_back, d + o_back, n_back, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    if (writes_pred)
        unpack_rows(pred, (ptrdiff_t)p_stride * sizeof(T), hb + o_out, (size_t)p_width * sizeof(T), p_height);
    else
        unpack_rows(conv_dst, (ptrdiff_t)conv_dst_stride * 2, hb + o_conv, (size_t)p_width * 2, p_height);
    return SVTGPU_OK;
}

} // namespace

extern "C" int svtgpu_warp_shear_params(const int32_t wmmat[6], int16_t abgd[4]) {
    if (!wmmat || !abgd) return SVTGPU_ERR_INVALID_ARG;
    return wp::shear_params(wmmat, abgd);
}

extern "C" int svtgpu_warp_filter_table(const int16_t **table, int32_t *rows) {
    if (!table || !rows) return SVTGPU_ERR_INVALID_ARG;
    *table = &wp::kFilter.row[0][0], *rows = wp::kFilterRows;
    return SVTGPU_OK;
}

extern "C" int svtgpu_warp_predict_batch(SvtGpuTfState *s, const SvtGpuTfPlanes *refs, int32_t n_refs, const SvtGpuWarpBlock *blocks,
                                         int32_t n_blocks, int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred,
                                         void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!batch_args_ok(s, refs, n_refs, blocks, n_blocks, bit_depth, pred)) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    // the kernel clamps every read into the picture: no border
    if (!check_planes(refs, n_refs, pred, width, 0, bit_depth, chroma ? 3 : 1)) return SVTGPU_ERR_INVALID_ARG;
    std::vector<DevBlock> dev((size_t)n_blocks);
    std::vector<WarpItem> items;
    for (int i = 0; i < n_blocks; i++) {
        const SvtGpuWarpBlock &b = blocks[i];
        const bool             two = b.ref1 != kNoRef;
        if (!check_block_rect(b.x, b.y, b.w_log2, b.h_log2, 8, width, height) || b.ref0 >= n_refs ||
            (two && (b.ref1 >= n_refs || !dist_wtd_ok(b.dist_wtd, b.fwd_offset, b.bck_offset))))
            return SVTGPU_ERR_INVALID_ARG;
        DevBlock &d = dev[(size_t)i];
        memset(&d, 0, sizeof d);
        d.x = b.x, d.y = b.y, d.w_log2 = b.w_log2, d.h_log2 = b.h_log2, d.ref0 = b.ref0, d.ref1 = b.ref1;
        d.dist_wtd = two ? b.dist_wtd : 0, d.fwd_offset = b.fwd_offset, d.bck_offset = b.bck_offset;
        const int bw = 1 << b.w_log2, bh = 1 << b.h_log2;
        for (int r = 0; r < (two ? 2 : 1); r++) {
            const int32_t *mat = r ? b.wmmat1 : b.wmmat0;
            memcpy(d.m[r].mat, mat, sizeof d.m[r].mat);
            if (wp::shear_params(mat, d.m[r].abgd) != 1) return SVTGPU_ERR_INVALID_ARG;
            // linear in the unit's position: the corner units bound every unit of the block, luma and chroma
            for (int c = 0; c < 4; c++) {
                int64_t dx, dy;
                if (!project(mat, 0, 0, b.x + ((c & 1) ? bw - 8 : 0), b.y + ((c & 2) ? bh - 8 : 0), &dx, &dy)) return SVTGPU_ERR_INVALID_ARG;
            }
        }
        warp_items((uint32_t)i, b.w_log2, b.h_log2, chroma != 0, [&](const WarpItem &it) { items.push_back(it); });
    }
    if (!n_blocks) return SVTGPU_OK;
    hipStream_t      st = pick_stream(ctx, stream);
    const MetaLayout lay((size_t)n_refs, (size_t)n_blocks, sizeof(DevBlock), items.size(), sizeof(WarpItem));
    uint8_t         *dm;
    if (int rc = meta_upload(s, lay, refs, dev.data(), st, &dm, items.data(), lay.item_bytes)) return rc;
    WarpArgs a;
    memset(&a, 0, sizeof a);
    a.refs = (const SvtGpuTfPlanes *)dm, a.blocks = (const DevBlock *)(dm + lay.o_blk), a.items = (const WarpItem *)(dm + lay.o_item);
    a.pred = *pred, a.width = width, a.height = height, a.bd = bit_depth;
    return launch_by_depth(bit_depth, warp_kernel<uint8_t>, warp_kernel<uint16_t>, dim3((unsigned)items.size()), dim3(256), st,
                           a);
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous.  svtgpu_rtcd.h's adapters spell the reference's ConvolveParams out.
// ---------------------------------------------------------------------------------------------
extern "C" int svtgpu_av1_warp_affine(const int32_t *mat, const uint8_t *ref, int32_t width, int32_t height, int32_t stride, uint8_t *pred,
                                      int32_t p_col, int32_t p_row, int32_t p_width, int32_t p_height, int32_t p_stride,
                                      int32_t subsampling_x, int32_t subsampling_y, int32_t round_0, int32_t round_1, int32_t is_compound,
                                      uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg,
                                      int32_t fwd_offset, int32_t bck_offset, int16_t alpha, int16_t beta, int16_t gamma, int16_t delta) {
    return shim_warp<uint8_t>(mat, ref, nullptr, width, height, stride, 0, pred, p_col, p_row, p_width, p_height, p_stride, subsampling_x,
                              subsampling_y, 8, round_0, round_1, is_compound, conv_dst, conv_dst_stride, do_average, use_jnt_comp_avg,
                              fwd_offset, bck_offset, alpha, beta, gamma, delta);
}
extern "C" int svtgpu_av1_highbd_warp_affine(const int32_t *mat, const uint8_t *ref8b, const uint8_t *ref2b, int32_t width, int32_t height,
                                             int32_t stride8b, int32_t stride2b, uint16_t *pred, int32_t p_col, int32_t p_row,
                                             int32_t p_width, int32_t p_height, int32_t p_stride, int32_t subsampling_x,
                                             int32_t subsampling_y, int32_t bd, int32_t round_0, int32_t round_1, int32_t is_compound,
                                             uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg,
                                             int32_t fwd_offset, int32_t bck_offset, int16_t alpha, int16_t beta, int16_t gamma,
                                             int16_t delta) {
    return shim_warp<uint16_t>(mat, ref8b, ref2b, width, height, stride8b, stride2b, pred, p_col, p_row, p_width, p_height, p_stride,
                               subsampling_x, subsampling_y, bd, round_0, round_1, is_compound, conv_dst, conv_dst_stride, do_average,
                               use_jnt_comp_avg, fwd_offset, bck_offset, alpha, beta, gamma, delta);
}
