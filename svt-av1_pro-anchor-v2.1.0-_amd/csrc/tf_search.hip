// tf_search.hip — the sub-pel motion search of the encoder's temporal filter on gfx950: the `frame_index != index_center`
// section of produce_temporally_filtered_pic (EbTemporalFiltering.c:3087-3261) minus ME and minus the two
// tf_*_inter_prediction calls, for every (reference, 64x64 block) of a picture as one launch, and err32 of the blocks that
// end on the 64x64 path (convert_64x64_info_to_32x32_info, :2665-2733) as a second small kernel behind the compensation.
//
//   tf_search_kernel  a workgroup owns one (reference, 64x64 block), a wave the 32x32 block idx_32x32 = the wave, as
//                     tf_predict_kernel and tf_frame_kernel map them.  The wave keeps its 32x32 quarter of the centre block
//                     in LDS and runs up to ten steps of one routine (search_step): its quarter of the 64x64 search (the
//                     four waves' moments combined through LDS, one workgroup barrier per position), its 32x32 search,
//                     its four 16x16 searches, and its sixteen 8x8 searches four at a time (16 lanes each).  A step stages
//                     the (b + 8)^2 window of the reference once -- every position of the walk lies within 7/8 sample of
//                     the full-pel start, whose clamped form has phase 0 -- with every coordinate clamped into the readable
//                     border, then walks the 25 positions in the reference's order under its skip rules.  A lane computes
//                     four adjacent samples of a row from eleven window samples; with sub_sampling_shift only the rows the
//                     variance reads are filtered (the C's sub-sampled centre prediction holds the same samples on them).
//   tf_err64_kernel   a workgroup per (reference, 64x64 block) that took the 64x64 path, a wave per 32x32 quadrant: the
//                     variance of the final predictor against the centre into the block record's err32.
//
// Arithmetic kept from the C: svt_check_position / tf_subpel_search (:1535-1765) -- centre first, then +-4, +-2, +-1 with x
// outer and y inner, diagonals dropped from mode 2, a position skipped when the best is 0 or below (b * b * th) <<
// is_highbd (32-bit), strict < so the first position wins a tie, the start INT_MAX; the MV held in int16, times two in
// int16, clamped as clamp_mv_to_umv_border_sb with the edges of each tf_*_sub_pel_search; the convolve form by the phases
// (copy / x / y / 2d) with get_conv_params_no_round's rounds 3 / 11 and the 8-bit 2-D result held in int16; vf = sse -
// sum^2 / n in uint32, vf_hbd_10 = rounded sse >> 4, rounded sum >> 2 (signed), clamped at 0; the distortion shifted left
// by sub_sampling_shift in 32 bits; the 64-vs-32 test in uint64; derive_tf_32x32_block_split_flag (:240-289) in int.
//
// Bounds: reference reads go through clamp_i into [-border, size + border - 1]; the centre is read over the 64-aligned
// area; window columns and rows are x + off + 1 + k with off in {-1, 0} (clamped so), k < 8, x < rs: below rs + 8; the
// intermediate holds (rs + 7) * rs <= 39 * 32 per group; record index r * nblk + block < n_refs * nblk.
#include <cstddef>
#include <cstring>

#include "conv_device.h"
#include "interp_tables.h"
#include "svtgpu_internal.h"

static_assert(sizeof(SvtGpuTfFullpel) == 352 && sizeof(SvtGpuTfSearchParams) == 40, "search records");
static_assert(sizeof(SvtGpuTfMotion) == 368 && sizeof(SvtGpuTfBlock) == 256, "search outputs");
static_assert(offsetof(SvtGpuTfFullpel, mv32_x) == 4 && offsetof(SvtGpuTfFullpel, mv16_x) == 20 &&
                  offsetof(SvtGpuTfFullpel, mv8_x) == 84 && offsetof(SvtGpuTfFullpel, force64) == 340,
              "SvtGpuTfFullpel's members are packed in declaration order");

namespace {

using namespace conv_device;

constexpr int      kMaxRefs = 26;
constexpr int      kWin     = 40; // 32 + 8
constexpr uint32_t kIntMax  = 0x7fffffffu;

struct SearchArgs {
    const void            *centre;
    const SvtGpuTfLuma    *refs;    // [n_refs]
    const SvtGpuTfFullpel *fullpel; // [n_refs][nblk]
    SvtGpuTfMotion        *motion;
    SvtGpuTfBlock         *blocks;
    uint64_t               th32;
    int32_t                cstride, blk_cols, nblk, width, height, border_x, border_y, bd;
    int32_t                mode[3], use_2tap, shift, enable8, early_th;
};

template <typename T> struct alignas(16) WaveLds {
    T        cen[32 * 32];    // the wave's quarter of the centre block
    T        win[kWin * kWin]; // the window(s) of the current step
    int16_t  im[39 * 32];     // the horizontal pass of the 2-D form
    int16_t  mv16[4][2], mv8[16][2];
    uint32_t err16[4];
    int32_t  err8[4]; // the sum over the four 8x8 blocks of a 16x16 block
};
struct Combine { // the 64x64 search's moments and the 32x32 errors, across the four waves
    uint32_t sse[2][4];
    int32_t  sum[2][4];
    uint32_t err32[4];
};

// vf / vf_hbd_10 of n = 1 << ln samples, then << shift in 32 bits
__device__ __forceinline__ uint32_t variance(uint64_t sse, int64_t sum, int ln, bool hbd, int shift) {
    uint32_t v;
    if (!hbd) {
        v = (uint32_t)sse - (uint32_t)((sum * sum) >> ln);
    } else {
        const uint32_t s = (uint32_t)((sse + 8) >> 4);
        const int      m = (int)((sum + 2) >> 2);
        const int64_t  d = (int64_t)s - (((int64_t)m * m) >> ln);
        v                = d >= 0 ? (uint32_t)d : 0;
    }
    return v << shift;
}

// What a lane knows of the block its group searches in this step.  rs, L and combine are wave-uniform.
struct Step {
    int rs, lrs;    // the region a group filters: rs x rs samples (the block itself but for the 64x64 search: its quarter)
    int L;          // lanes of a group: 64, or 16 for the 8x8 blocks (four groups side by side)
    int sub;        // the lane within its group
    int win, im;    // the group's window (row stride rs + 8) and intermediate (row stride rs) in the wave's LDS
    int cen;        // the region's top-left sample in the wave's centre quarter (row stride 32)
    int px, py, b;  // the prediction block: its origin in the picture and its size (the MV clamp, the variance's n)
    int ox, oy;     // the region's origin in the picture
    int tab;        // the filter table
    int mvx, mvy;   // in: the start MV in 1/8 sample; out: the best
    uint32_t best;  // out
    bool combine;   // the 64x64 search: the moments of the four waves are added
};

template <typename T>
__device__ __forceinline__ void search_step(const SearchArgs &a, const T *__restrict__ ref, int rstride, WaveLds<T> *lds,
                                            Combine *cmb, int wave, Step &d, int &nev) {
    const int  ww = d.rs + 8, g4 = d.rs >> 2, lg4 = d.lrs - 2;
    const bool hbd = a.bd > 8;
    const int  spel = (4 + d.b) << 4;
    const int  lo_x = -(d.px * 16) - spel, hi_x = (a.width - d.b - d.px) * 16 + spel - 16;
    const int  lo_y = -(d.py * 16) - spel, hi_y = (a.height - d.b - d.py) * 16 + spel - 16;
    // the clamped start has phase 0: the window's column 4 / row 4 is its integer position
    const int base_x = (int16_t)clamp_i((int16_t)(d.mvx * 2), lo_x, hi_x) >> 4;
    const int base_y = (int16_t)clamp_i((int16_t)(d.mvy * 2), lo_y, hi_y) >> 4;
    wave_lds_sync(); // the previous step's reads before this step's stores
    {
        const int recip = (1 << 20) / ww + 1; // i / ww exactly for ww in {16, 24, 40} and i < ww * ww
        for (int i = d.sub; i < ww * ww; i += d.L) {
            const int y = (i * recip) >> 20, x = i - y * ww;
            const int gx = clamp_i(d.ox + base_x - 4 + x, -a.border_x, a.width + a.border_x - 1);
            const int gy = clamp_i(d.oy + base_y - 4 + y, -a.border_y, a.height + a.border_y - 1);
            lds->win[d.win + i] = ref[(ptrdiff_t)gy * rstride + gx];
        }
    }
    wave_lds_sync();
    const uint32_t thr   = ((uint32_t)(d.b * d.b) * (uint32_t)a.early_th) << (hbd ? 1 : 0);
    const int      ln    = 2 * (31 - __clz(d.b)) - a.shift; // log2 of b * (b >> shift)
    const int      ymask = (1 << a.shift) - 1;
    uint32_t       best  = kIntMax;
    int            bmx = d.mvx, bmy = d.mvy, sx = d.mvx, sy = d.mvy;
#pragma unroll 1
    for (int pos = 0; pos < 25; pos++) {
        int  dx = 0, dy = 0;
        bool active = true;
        if (pos > 0) {
            const int s = (pos - 1) >> 3, p = (pos - 1) & 7, md = a.mode[s];
            if (!md) {
                pos += 7;
                continue;
            }
            if (p == 0) sx = bmx, sy = bmy;
            const int k = p + (p >= 4), i = k / 3 - 1, j = k - 3 * (k / 3) - 1;
            dx = i * (4 >> s), dy = j * (4 >> s);
            active = !(md >= 2 && i && j) && best != 0 && !(a.early_th && best < thr);
        }
        if (!__any(active)) continue; // uniform over the wave, and over the workgroup in the 64x64 search
        const int mvx = (int16_t)(sx + dx), mvy = (int16_t)(sy + dy);
        const int qx = (int16_t)clamp_i((int16_t)(mvx * 2), lo_x, hi_x), qy = (int16_t)clamp_i((int16_t)(mvy * 2), lo_y, hi_y);
        const int phx = qx & 15, phy = qy & 15;
        const int offx = clamp_i((qx >> 4) - base_x, -1, 0), offy = clamp_i((qy >> 4) - base_y, -1, 0);
        int       fx[8], fy[8];
        {
            const int4 tx = *(const int4 *)kInterpFilters[d.tab][phx], ty = *(const int4 *)kInterpFilters[d.tab][phy];
            fx[0] = (int16_t)tx.x, fx[1] = tx.x >> 16, fx[2] = (int16_t)tx.y, fx[3] = tx.y >> 16;
            fx[4] = (int16_t)tx.z, fx[5] = tx.z >> 16, fx[6] = (int16_t)tx.w, fx[7] = tx.w >> 16;
            fy[0] = (int16_t)ty.x, fy[1] = ty.x >> 16, fy[2] = (int16_t)ty.y, fy[3] = ty.y >> 16;
            fy[4] = (int16_t)ty.z, fy[5] = ty.z >> 16, fy[6] = (int16_t)ty.w, fy[7] = ty.w >> 16;
        }
        const T *win = lds->win + d.win;
        if (phx && phy) { // the horizontal pass of the 2-D form: rs + 7 rows
            for (int i = d.sub; i < (d.rs + 7) * g4; i += d.L) {
                const int r = i >> lg4, x4 = (i & (g4 - 1)) * 4;
                const T  *p = win + (r + offy + 1) * ww + x4 + offx + 1;
                int       v[11];
#pragma unroll
                for (int k = 0; k < 11; k++) v[k] = p[k];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    int s = 1 << (a.bd + 6);
#pragma unroll
                    for (int k = 0; k < 8; k++) s += fx[k] * v[o + k];
                    lds->im[d.im + r * d.rs + x4 + o] = (int16_t)round_shift(s, 3);
                }
            }
        }
        wave_lds_sync();
        uint32_t sse = 0;
        int      sum = 0;
        for (int i = d.sub; i < d.rs * g4; i += d.L) {
            const int y = i >> lg4, x4 = (i & (g4 - 1)) * 4;
            if (y & ymask) continue;
            int pr[4];
            if (phx && phy) {
                const int16_t *p = lds->im + d.im + y * d.rs + x4;
                const int      offset_bits = a.bd + 11, sub = (1 << (offset_bits - 11)) + (1 << (offset_bits - 12));
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    int s = 1 << offset_bits;
#pragma unroll
                    for (int k = 0; k < 8; k++) s += fy[k] * (int)p[k * d.rs + o];
                    int res = round_shift(s, 11) - sub;
                    if (sizeof(T) == 1) res = (int16_t)res;
                    pr[o] = clip_bd(res, a.bd); // the last rounding is by 14 - 3 - 11 = 0 bits
                }
            } else if (phx) {
                const T *p = win + (y + offy + 4) * ww + x4 + offx + 1;
                int      v[11];
#pragma unroll
                for (int k = 0; k < 11; k++) v[k] = p[k];
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    int s = 0;
#pragma unroll
                    for (int k = 0; k < 8; k++) s += fx[k] * v[o + k];
                    pr[o] = clip_bd(round_shift(round_shift(s, 3), 4), a.bd);
                }
            } else if (phy) {
                const T *p = win + (y + offy + 1) * ww + x4 + offx + 4;
#pragma unroll
                for (int o = 0; o < 4; o++) {
                    int s = 0;
#pragma unroll
                    for (int k = 0; k < 8; k++) s += fy[k] * (int)p[k * ww + o];
                    pr[o] = clip_bd(round_shift(s, 7), a.bd);
                }
            } else {
                const T *p = win + (y + offy + 4) * ww + x4 + offx + 4;
#pragma unroll
                for (int o = 0; o < 4; o++) pr[o] = p[o];
            }
            const T *c = lds->cen + d.cen + y * 32 + x4;
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int df = pr[o] - (int)c[o];
                sum += df, sse += (uint32_t)(df * df);
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1)
            if (m < d.L) sse += (uint32_t)__shfl_xor((int)sse, m, 64), sum += __shfl_xor(sum, m, 64);
        uint64_t tsse = sse;
        int64_t  tsum = sum;
        if (d.combine) {
            const int par = nev & 1;
            if (d.sub == 0) cmb->sse[par][wave] = sse, cmb->sum[par][wave] = sum;
            __syncthreads();
            tsse = (uint64_t)cmb->sse[par][0] + cmb->sse[par][1] + cmb->sse[par][2] + cmb->sse[par][3];
            tsum = (int64_t)cmb->sum[par][0] + cmb->sum[par][1] + cmb->sum[par][2] + cmb->sum[par][3];
        }
        nev++;
        const uint32_t dist = variance(tsse, tsum, ln, hbd, a.shift);
        if (active && dist < best) best = dist, bmx = mvx, bmy = mvy;
        wave_lds_sync(); // this position's reads of win / im before the next position's horizontal-pass stores
    }
    d.best = best, d.mvx = bmx, d.mvy = bmy;
}

template <typename T>
__global__ __launch_bounds__(256) void tf_search_kernel(const SearchArgs a) {
    __shared__ WaveLds<T> lds_all[4];
    __shared__ Combine    cmb;
    const int   lane = threadIdx.x & 63, idx = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int   r = blockIdx.x / a.nblk, blk = blockIdx.x - r * a.nblk;
    const int   bx = (blk % a.blk_cols) * 64, by = (blk / a.blk_cols) * 64;
    const int   qx = bx + (idx & 1) * 32, qy = by + (idx >> 1) * 32;
    WaveLds<T> *lds = &lds_all[idx];
    const T    *ref = (const T *)a.refs[r].plane;
    const int   rstride = a.refs[r].stride;
    const size_t           rec = (size_t)r * a.nblk + blk;
    const SvtGpuTfFullpel &fp  = a.fullpel[rec];
    SvtGpuTfMotion        &mo  = a.motion[rec];
    SvtGpuTfBlock         &bl  = a.blocks[rec];

    { // the centre quarter: 16-byte row pieces
        constexpr int per_row = 32 * sizeof(T) / 16;
        for (int i = lane; i < 32 * per_row; i += 64) {
            const int y = i / per_row, c = i % per_row;
            const uint4 v = *(const uint4 *)((const T *)a.centre + (size_t)(qy + y) * a.cstride + qx + c * (16 / sizeof(T)));
            *(uint4 *)(lds->cen + y * 32 + c * (16 / sizeof(T))) = v;
        }
    }
    int  nev = 0;
    Step d;
    d.L = 64, d.sub = lane, d.win = 0, d.im = 0;

    // the 64x64 search: this wave's quarter
    d.rs = 32, d.lrs = 5, d.cen = 0, d.px = bx, d.py = by, d.b = 64, d.ox = qx, d.oy = qy, d.combine = true;
    d.tab = a.use_2tap ? kInterpBilinear : kInterpRegular;
    d.mvx = (int16_t)(fp.mv64_x * 8), d.mvy = (int16_t)(fp.mv64_y * 8);
    search_step<T>(a, ref, rstride, lds, &cmb, idx, d, nev);
    const uint32_t err64 = d.best;
    const int      mv64x = d.mvx, mv64y = d.mvy;
    bool           use64 = fp.force64 != 0;
    uint32_t       err32 = 0;
    int            mv32x = 0, mv32y = 0;
    if (!use64) {
        d.px = qx, d.py = qy, d.b = 32, d.combine = false;
        d.mvx = (int16_t)(fp.mv32_x[idx] * 8), d.mvy = (int16_t)(fp.mv32_y[idx] * 8);
        search_step<T>(a, ref, rstride, lds, &cmb, idx, d, nev);
        err32 = d.best, mv32x = d.mvx, mv32y = d.mvy;
        if (lane == 0) cmb.err32[idx] = err32;
        __syncthreads();
        const uint64_t sum32 = (uint64_t)cmb.err32[0] + cmb.err32[1] + cmb.err32[2] + cmb.err32[3];
        use64 = (uint64_t)err64 * 14 < sum32 * 16 && err64 < (1u << 18);
    }
    if (use64) { // everything else of the records stays 0; err32 comes from tf_err64_kernel
        if (lane == 0) {
            if (idx == 0) mo.use64 = 1, mo.mv64_x = (int16_t)mv64x, mo.mv64_y = (int16_t)mv64y;
            bl.mv32_x[idx] = (int16_t)mv64x, bl.mv32_y[idx] = (int16_t)mv64y;
        }
        return;
    }
    bool split32 = false;
    int  split16 = 0, e16[4] = {0, 0, 0, 0};
    if (!((uint64_t)err32 < a.th32)) {
        d.rs = 16, d.lrs = 4, d.b = 16, d.tab = kInterpRegular;
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            d.px = d.ox = qx + (j & 1) * 16, d.py = d.oy = qy + (j >> 1) * 16, d.cen = (j >> 1) * 16 * 32 + (j & 1) * 16;
            d.mvx = (int16_t)(fp.mv16_x[idx * 4 + j] * 8), d.mvy = (int16_t)(fp.mv16_y[idx * 4 + j] * 8);
            search_step<T>(a, ref, rstride, lds, &cmb, idx, d, nev);
            if (lane == 0) lds->err16[j] = d.best, lds->mv16[j][0] = (int16_t)d.mvx, lds->mv16[j][1] = (int16_t)d.mvy;
        }
        if (a.enable8) {
            const int k = lane >> 4; // the 8x8 block of the lane's group
            d.rs = 8, d.lrs = 3, d.b = 8, d.L = 16, d.sub = lane & 15, d.win = k * 256, d.im = k * 120;
#pragma unroll 1
            for (int j = 0; j < 4; j++) {
                const int x8 = (j & 1) * 16 + (k & 1) * 8, y8 = (j >> 1) * 16 + (k >> 1) * 8, i8 = idx * 16 + j * 4 + k;
                d.px = d.ox = qx + x8, d.py = d.oy = qy + y8, d.cen = y8 * 32 + x8;
                d.mvx = (int16_t)(fp.mv8_x[i8] * 8), d.mvy = (int16_t)(fp.mv8_y[i8] * 8);
                search_step<T>(a, ref, rstride, lds, &cmb, idx, d, nev);
                int e = (int)d.best; // the four groups' errors, added in int as the C adds them
                e += __shfl_xor(e, 16, 64), e += __shfl_xor(e, 32, 64);
                if (d.sub == 0) lds->mv8[j * 4 + k][0] = (int16_t)d.mvx, lds->mv8[j * 4 + k][1] = (int16_t)d.mvy;
                if (lane == 0) lds->err8[j] = e;
            }
        }
        wave_lds_sync();
        // derive_tf_32x32_block_split_flag
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int e = (int)lds->err16[j];
            if (a.enable8) {
                const int e8 = lds->err8[j];
                if (!(e * 8 < e8 * 16)) split16 |= 1 << j, e = e8;
            }
            e16[j] = e, sum += e;
        }
        split32 = !((int)err32 * 14 < sum * 16);
    }
    if (lane != 0) return;
    if (!split32) {
        mo.mv32_x[idx] = bl.mv32_x[idx] = (int16_t)mv32x, mo.mv32_y[idx] = bl.mv32_y[idx] = (int16_t)mv32y;
        bl.err32[idx] = err32;
        return;
    }
    mo.split32[idx] = 1, bl.split32[idx] = 1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int     q = idx * 4 + j;
        const int16_t x = lds->mv16[j][0], y = lds->mv16[j][1];
        bl.mv16_x[q] = x, bl.mv16_y[q] = y, bl.err16[q] = (uint64_t)(int64_t)e16[j];
        if (split16 >> j & 1) {
            mo.split16[q] = 1;
            for (int k = 0; k < 4; k++) mo.mv8_x[q * 4 + k] = lds->mv8[j * 4 + k][0], mo.mv8_y[q * 4 + k] = lds->mv8[j * 4 + k][1];
        } else {
            mo.mv16_x[q] = x, mo.mv16_y[q] = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// err32 of the blocks on the 64x64 path
// ---------------------------------------------------------------------------------------------
struct Err64Args {
    const void           *centre;
    const SvtGpuTfLuma   *pred; // [n_refs]
    const SvtGpuTfMotion *motion;
    SvtGpuTfBlock        *blocks;
    int32_t               cstride, blk_cols, nblk, shift, hbd;
};
template <typename T>
__global__ __launch_bounds__(256) void tf_err64_kernel(const Err64Args a) {
    const int    lane = threadIdx.x & 63, idx = threadIdx.x >> 6;
    const int    r = blockIdx.x / a.nblk, blk = blockIdx.x - r * a.nblk;
    const size_t rec = (size_t)r * a.nblk + blk;
    if (!a.motion[rec].use64) return;
    const int x0 = (blk % a.blk_cols) * 64 + (idx & 1) * 32, y0 = (blk / a.blk_cols) * 64 + (idx >> 1) * 32;
    const T  *pr = (const T *)a.pred[r].plane, *ce = (const T *)a.centre;
    const int ps = a.pred[r].stride;
    uint32_t  sse = 0;
    int       sum = 0;
    for (int i = lane; i < 32 * 32; i += 64) {
        const int y = i >> 5, x = i & 31;
        if (y & ((1 << a.shift) - 1)) continue;
        const int df = (int)pr[(size_t)(y0 + y) * ps + x0 + x] - (int)ce[(size_t)(y0 + y) * a.cstride + x0 + x];
        sum += df, sse += (uint32_t)(df * df);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sse += (uint32_t)__shfl_xor((int)sse, m, 64), sum += __shfl_xor(sum, m, 64);
    if (lane == 0) a.blocks[rec].err32[idx] = variance(sse, sum, 10 - a.shift, a.hbd != 0, a.shift);
}

bool param_ok(int v, int lo, int hi) { return v >= lo && v <= hi; }
// 2047 * 8 + 7, doubled, is the reference's int16 at its end
bool mv_ok(const int16_t *v, int n) {
    for (int i = 0; i < n; i++)
        if (v[i] < -2047 || v[i] > 2047) return false;
    return true;
}
bool fullpel_ok(const SvtGpuTfFullpel &f) {
    return mv_ok(&f.mv64_x, 1) && mv_ok(&f.mv64_y, 1) && mv_ok(f.mv32_x, 4) && mv_ok(f.mv32_y, 4) && mv_ok(f.mv16_x, 16) &&
        mv_ok(f.mv16_y, 16) && mv_ok(f.mv8_x, 64) && mv_ok(f.mv8_y, 64);
}

} // namespace

int svtgpu_tf_err64_launch(SvtGpuTfState *s, const SvtGpuTfPlanes *centre, const SvtGpuTfLuma *d_pred,
                           const SvtGpuTfMotion *d_motion, SvtGpuTfBlock *d_blocks, int n_refs, int bit_depth,
                           int sub_sampling_shift, hipStream_t st) {
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    Err64Args a;
    a.centre = centre->plane[0], a.cstride = centre->stride[0], a.pred = d_pred, a.motion = d_motion, a.blocks = d_blocks;
    a.blk_cols = blk_cols, a.nblk = nblk, a.shift = sub_sampling_shift, a.hbd = bit_depth > 8;
    const dim3 grid((unsigned)(n_refs * nblk));
    if (bit_depth == 8)
        hipLaunchKernelGGL(tf_err64_kernel<uint8_t>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(tf_err64_kernel<uint16_t>, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

extern "C" int svtgpu_tf_search_frame(SvtGpuTfState *s, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs,
                                      int32_t n_refs, int32_t border_x, int32_t border_y, const SvtGpuTfFullpel *fullpel,
                                      const SvtGpuTfSearchParams *p, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!s || !centre || !p || n_refs < 0 || (n_refs && (!refs || !fullpel)) || (p->bit_depth != 8 && p->bit_depth != 10) ||
        border_x < 0 || border_y < 0 || !param_ok(p->half_pel_mode, 0, 2) || !param_ok(p->quarter_pel_mode, 0, 2) ||
        !param_ok(p->eight_pel_mode, 0, 2) || !param_ok(p->use_2tap, 0, 1) || !param_ok(p->sub_sampling_shift, 0, 1) ||
        !param_ok(p->enable_8x8_pred, 0, 1) || !param_ok(p->subpel_early_exit_th, 0, 255))
        return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    const int bs = p->bit_depth > 8 ? 2 : 1, aw = blk_cols * 64;
    if (!centre->plane[0] || centre->stride[0] < aw || (((size_t)centre->stride[0] * bs) & 15) || ((uintptr_t)centre->plane[0] & 15))
        return SVTGPU_ERR_INVALID_ARG;
    for (int r = 0; r < n_refs; r++)
        if (!refs[r].plane[0] || ((uintptr_t)refs[r].plane[0] & (bs - 1)) || refs[r].stride[0] < width + 2 * border_x)
            return SVTGPU_ERR_INVALID_ARG;
    const size_t nrec = (size_t)n_refs * nblk;
    for (size_t k = 0; k < nrec; k++)
        if (!fullpel_ok(fullpel[k])) return SVTGPU_ERR_INVALID_ARG;
    svtgpu_tf_records_commit(s, 0); // the previous search's records end here; the count returns once this one is queued
    if (!n_refs) return SVTGPU_OK;
    hipStream_t  st  = pick_stream(ctx, stream);
    const size_t off = ((size_t)n_refs * sizeof(SvtGpuTfLuma) + 15) & ~(size_t)15, nb = nrec * sizeof(SvtGpuTfFullpel);
    uint8_t     *hm, *dm;
    SearchArgs   a;
    if (int rc = svtgpu_tf_records_reserve(s, n_refs, &a.motion, &a.blocks)) return rc;
    if (int rc = svtgpu_tf_meta_begin(s, off + nb, &hm, &dm)) return rc;
    SvtGpuTfLuma *hl = (SvtGpuTfLuma *)hm;
    for (int r = 0; r < n_refs; r++) hl[r].plane = refs[r].plane[0], hl[r].stride = refs[r].stride[0], hl[r].pad = 0;
    memcpy(hm + off, fullpel, nb);
    if (int rc = svtgpu_tf_meta_upload(s, off + nb, st)) return rc;
    svtgpu_tf_records_commit(s, n_refs);
    // the kernel writes only what a consumer reads under the block's flags: everything else is 0
    HIP_TRY(hipMemsetAsync(a.motion, 0, nrec * sizeof(SvtGpuTfMotion), st));
    HIP_TRY(hipMemsetAsync(a.blocks, 0, nrec * sizeof(SvtGpuTfBlock), st));
    a.centre = centre->plane[0], a.cstride = centre->stride[0];
    a.refs = (const SvtGpuTfLuma *)dm, a.fullpel = (const SvtGpuTfFullpel *)(dm + off);
    a.th32 = p->pred_error_32x32_th;
    a.blk_cols = blk_cols, a.nblk = nblk, a.width = width, a.height = height, a.border_x = border_x, a.border_y = border_y;
    a.bd = p->bit_depth, a.mode[0] = p->half_pel_mode, a.mode[1] = p->quarter_pel_mode, a.mode[2] = p->eight_pel_mode;
    a.use_2tap = p->use_2tap, a.shift = p->sub_sampling_shift, a.enable8 = p->enable_8x8_pred, a.early_th = p->subpel_early_exit_th;
    if (bs == 1)
        hipLaunchKernelGGL(tf_search_kernel<uint8_t>, dim3((unsigned)nrec), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(tf_search_kernel<uint16_t>, dim3((unsigned)nrec), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

extern "C" int svtgpu_tf_search_read(SvtGpuTfState *s, int32_t n_refs, SvtGpuTfMotion *motion_out, SvtGpuTfBlock *blocks_out,
                                     void *stream) {
    if (!s || !motion_out || !blocks_out || n_refs <= 0) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuTfMotion *dmo;
    SvtGpuTfBlock  *dbl;
    if (svtgpu_tf_records_get(s, &dmo, &dbl) != n_refs) return SVTGPU_ERR_INVALID_ARG;
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    svtgpu_tf_state_geometry(s, &ctx, &width, &height, &blk_cols, &nblk);
    hipStream_t  st = pick_stream(ctx, stream);
    const size_t n  = (size_t)n_refs * nblk;
    HIP_TRY(hipMemcpyAsync(motion_out, dmo, n * sizeof(SvtGpuTfMotion), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(blocks_out, dbl, n * sizeof(SvtGpuTfBlock), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    svtgpu_count_xfer(1, n * (sizeof(SvtGpuTfMotion) + sizeof(SvtGpuTfBlock)));
    return SVTGPU_OK;
}
