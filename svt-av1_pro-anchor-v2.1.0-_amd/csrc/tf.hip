// tf.hip — the filter half of the encoder's temporal filter (EbTemporalFiltering.c) on gfx950: the noise estimate
// (svt_estimate_noise_fp16_c / svt_estimate_noise_highbd_fp16_c, :3672-3740), and the block loop of
// produce_temporally_filtered_pic (:2939-3301) from apply_filtering_central to get_final_filtered_pixels as one launch per
// picture.  The entry takes what the motion half leaves behind, the predictor pictures and one SvtGpuTfBlock per
// (reference, 64x64 block): from the host (svtgpu_tf_filter_frame), or from the device records of tf_search.hip with the
// compensation of interp.hip in front (svtgpu_tf_compensate_filter_frame); only HME / ME stays on the host.
//
//   tf_frame_kernel   a workgroup owns a 64x64 block (luma and both chroma), a wave one 32x32 block of it (idx_32x32 =
//                     the wave).  A lane holds 2 x 8 adjacent luma samples (rows l >> 2 and 16 + (l >> 2), columns
//                     8 * (l & 3)) and 4 adjacent samples of each chroma plane, so bit 1 of the lane is the quadrant's
//                     column and the luma pass / bit 5 its row.  The centre samples and `accum` stay in registers over
//                     the reference loop; a weight is uniform over a 16x16 quadrant, so `count` is one register per
//                     quadrant the lane touches.  Per reference and quadrant one SSE reduction over the lanes of that
//                     quadrant (xor butterflies that skip the quadrant bits).  The next reference's samples are loaded
//                     (16-B / 8-B per lane) before the current ones are reduced.  Nothing but the output is written:
//                     no accumulator or counter planes.
//   tf_noise_kernel   a grid-wide integer reduction (64-bit atomics; integer sums have no order), the last workgroup
//                     divides, so the frame-level form needs no host wait.
//   tf_block_kernel / tf_central_kernel / tf_final_kernel: the per-block RTCD shims' kernels, one small launch each.
//
// Integer arithmetic follows the reference's types: uint32 wrap-around where its C has uint32, and the avg_err product
// (combined >> 3) * (d_factor >> 3) is a 32-bit product (:1098).  OD_DIVU's table branch (count < 1024: the centre's 1000
// and references whose weights add up to at most 23) equals plain division for every accum the filter can form with such
// a count (the fixtures' generators check them all: divisor 1000 in gen_golden_tf.c, 1000 .. 1023 in
// gen_golden_tf_search.c --extreme), so the normalisation divides.
//
// Bounds: the frame kernel reads and writes the 64-aligned area only (the entry's contract), metadata index r * nblk +
// block < n_refs * nblk; the noise kernel guards every row and column against h and w; the shim kernels index packed
// buffers sized by the same w x h they loop over.
#include <cstring>
#include <vector>

#include "svtgpu_internal.h"
#include "tf_tables.h"

namespace {

using pred_plan::kMaxRefs;
constexpr uint32_t kTfWeight  = 1000; // TF_WEIGHT_SCALE, TF_PLANEWISE_FILTER_WEIGHT_SCALE
constexpr int      kExpfLast  = 7 * 16;

// ---------------------------------------------------------------------------------------------
// scalar arithmetic shared by the kernels and the host-only entries
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t tf_sqrt_fast(uint32_t x) { // sqrt_fast (:709-718)
    if (x > 15) {
#ifdef __HIP_DEVICE_COMPILE__
        const int log2_half = (31 - __clz((int)x)) >> 1;
#else
        const int log2_half = (31 - __builtin_clz(x)) >> 1;
#endif
        return kTfSqrtFp16[x >> (2 * log2_half - 2)] >> (17 - log2_half);
    }
    return kTfSqrtFp16[x] >> 16;
}
// distance_threshold_fp16 >> 8 of a tf_mv_dist_th (:1015)
inline uint32_t tf_threshold_shr8(int32_t mv_dist_th) {
    const int32_t t = (int32_t)(((uint32_t)mv_dist_th << 16) / 10);
    return (uint32_t)(t > (1 << 16) ? t : (1 << 16)) >> 8;
}
__host__ __device__ inline uint32_t tf_d_factor(int32_t col, int32_t row, uint32_t thr_shr8) {
    const uint32_t d = (tf_sqrt_fast(((uint32_t)(col * col + row * row)) << 8) << 12) / thr_shr8;
    return d > 256u ? d : 256u;
}
__host__ __device__ inline uint32_t tf_window_error(uint32_t sse, uint32_t bw_half, uint32_t bh_half, int shift) {
    return ((((sse >> shift) << 4) / bw_half) << 4) / bh_half;
}
__host__ __device__ inline uint32_t tf_weight(uint32_t window_fp8, uint32_t block_fp8, uint32_t d_factor, uint32_t decay) {
    const uint32_t combined = (window_fp8 * 5u + block_fp8) / 6u;
    const uint32_t avg_err  = (combined >> 3) * (d_factor >> 3); // 32 bits, as the reference's C
    const uint32_t div      = decay >> 10 ? decay >> 10 : 1u;
    uint32_t       sd       = avg_err / div;
    sd                      = sd < (uint32_t)kExpfLast ? sd : (uint32_t)kExpfLast;
    return ((uint32_t)kTfExpfFp16[sd] * kTfWeight) >> 16;
}
__host__ __device__ inline uint32_t tf_weight_zz(uint32_t block_fp8, uint32_t decay) {
    const uint32_t div = decay >> 10 ? decay >> 10 : 1u;
    uint32_t       sd  = (block_fp8 << 2) / div;
    sd                 = sd < (uint32_t)kExpfLast ? sd : (uint32_t)kExpfLast;
    return ((uint32_t)kTfExpfFp16[sd] * kTfWeight) >> 17;
}
// block_error_fp8 of quadrant q of 32x32 block idx
__host__ __device__ inline uint32_t tf_block_error(const SvtGpuTfBlock &b, int idx, int q, bool hbd) {
    return b.split32[idx] ? (uint32_t)(b.err16[idx * 4 + q] >> (hbd ? 4 : 0)) : (uint32_t)(b.err32[idx] >> (hbd ? 6 : 2));
}

__device__ __forceinline__ uint32_t xor_add(uint32_t v, int mask) { return v + (uint32_t)__shfl_xor((int)v, mask, 64); }
__device__ __forceinline__ uint32_t wave_total(uint32_t v) { // every lane gets the wave's sum (mod 2^32)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = xor_add(v, m);
    return v;
}

// ---------------------------------------------------------------------------------------------
// the frame kernel
// ---------------------------------------------------------------------------------------------
struct TfRef {
    const void *plane[3];
    int32_t     stride[3];
    int32_t     pad;
};
struct TfFrameArgs {
    const void          *centre[3];
    void                *out[3];
    int32_t              cstride[3], ostride[3];
    const TfRef         *refs;   // [n_refs]
    const SvtGpuTfBlock *blocks; // [n_refs][nblk]
    int32_t              n_refs, blk_cols, nblk;
    uint32_t             decay[3], thr_shr8;
    int32_t              tf_chroma, bd, zz;
};

template <typename T> struct Raw;
template <> struct Raw<uint16_t> {
    typedef uint4 Y; // 8 luma samples
    typedef uint2 C; // 4 chroma samples
    Y y[2];
    C u, v;
};
template <> struct Raw<uint8_t> {
    typedef uint2    Y;
    typedef uint32_t C;
    Y y[2];
    C u, v;
};
__device__ __forceinline__ void unpack_y(const uint4 &r, uint32_t o[8]) {
    o[0] = r.x & 0xffff, o[1] = r.x >> 16, o[2] = r.y & 0xffff, o[3] = r.y >> 16;
    o[4] = r.z & 0xffff, o[5] = r.z >> 16, o[6] = r.w & 0xffff, o[7] = r.w >> 16;
}
__device__ __forceinline__ void unpack_y(const uint2 &r, uint32_t o[8]) {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (r.x >> (8 * i)) & 0xff, o[4 + i] = (r.y >> (8 * i)) & 0xff;
}
__device__ __forceinline__ void unpack_c(const uint2 &r, uint32_t o[4]) {
    o[0] = r.x & 0xffff, o[1] = r.x >> 16, o[2] = r.y & 0xffff, o[3] = r.y >> 16;
}
__device__ __forceinline__ void unpack_c(uint32_t r, uint32_t o[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (r >> (8 * i)) & 0xff;
}
__device__ __forceinline__ void pack_y(const uint32_t o[8], uint4 *r) {
    *r = make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
}
__device__ __forceinline__ void pack_y(const uint32_t o[8], uint2 *r) {
    *r = make_uint2(o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24, o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24);
}
__device__ __forceinline__ void pack_c(const uint32_t o[4], uint2 *r) { *r = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16); }
__device__ __forceinline__ void pack_c(const uint32_t o[4], uint32_t *r) { *r = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24; }

template <typename T>
__device__ __forceinline__ Raw<T> load_raw(const void *const plane[3], const int32_t stride[3], int ly0, int lx, int cy, int cx,
                                            bool chroma) {
    typedef typename Raw<T>::Y Y;
    typedef typename Raw<T>::C C;
    Raw<T>   r;
    const T *py = (const T *)plane[0];
    r.y[0]      = *(const Y *)(py + (size_t)ly0 * stride[0] + lx);
    r.y[1]      = *(const Y *)(py + (size_t)(ly0 + 16) * stride[0] + lx);
    if (chroma) {
        r.u = *(const C *)((const T *)plane[1] + (size_t)cy * stride[1] + cx);
        r.v = *(const C *)((const T *)plane[2] + (size_t)cy * stride[2] + cx);
    } else {
        r.u = r.v = C{};
    }
    return r;
}

template <typename T>
__global__ __launch_bounds__(256) void tf_frame_kernel(const TfFrameArgs a) {
    const int  lane = threadIdx.x & 63, idx = threadIdx.x >> 6; // idx: the wave's 32x32 block
    const int  bx = blockIdx.x % a.blk_cols, by = blockIdx.x / a.blk_cols;
    const int  h = (lane >> 1) & 1, kc = lane >> 5; // the lane's quadrant column; its chroma quadrant row
    const int  ly0 = by * 64 + (idx >> 1) * 32 + (lane >> 2), lx = bx * 64 + (idx & 1) * 32 + (lane & 3) * 8;
    const int  cy = by * 32 + (idx >> 1) * 16 + (lane >> 2), cx = bx * 32 + (idx & 1) * 16 + (lane & 3) * 4;
    const bool chroma = a.tf_chroma != 0, hbd = a.bd > 8;
    const int  shift = 2 * (a.bd - 8);

    uint32_t cen_y[2][8], cen_u[4], cen_v[4];
    {
        const Raw<T> c = load_raw<T>(a.centre, a.cstride, ly0, lx, cy, cx, true);
        unpack_y(c.y[0], cen_y[0]), unpack_y(c.y[1], cen_y[1]), unpack_c(c.u, cen_u), unpack_c(c.v, cen_v);
    }
    uint32_t acc_y[2][8], acc_u[4], acc_v[4], cnt_y[2] = {kTfWeight, kTfWeight}, cnt_u = kTfWeight, cnt_v = kTfWeight;
#pragma unroll
    for (int i = 0; i < 8; i++) acc_y[0][i] = kTfWeight * cen_y[0][i], acc_y[1][i] = kTfWeight * cen_y[1][i];
#pragma unroll
    for (int i = 0; i < 4; i++) acc_u[i] = kTfWeight * cen_u[i], acc_v[i] = kTfWeight * cen_v[i];

    Raw<T> nxt;
    if (a.n_refs > 0) nxt = load_raw<T>(a.refs[0].plane, a.refs[0].stride, ly0, lx, cy, cx, chroma);
    for (int r = 0; r < a.n_refs; r++) {
        const Raw<T> cur = nxt;
        if (r + 1 < a.n_refs) nxt = load_raw<T>(a.refs[r + 1].plane, a.refs[r + 1].stride, ly0, lx, cy, cx, chroma);
        const SvtGpuTfBlock &b     = a.blocks[(size_t)r * a.nblk + blockIdx.x];
        const bool           split = b.split32[idx] != 0;
        uint32_t             py[2][8], pu[4], pv[4], wy[2], wu = 0, wv = 0;
        unpack_y(cur.y[0], py[0]), unpack_y(cur.y[1], py[1]), unpack_c(cur.u, pu), unpack_c(cur.v, pv);
        if (a.zz) {
#pragma unroll
            for (int k = 0; k < 2; k++) wy[k] = tf_weight_zz(tf_block_error(b, idx, 2 * k + h, hbd), a.decay[0]);
            if (chroma) {
                const uint32_t be = tf_block_error(b, idx, 2 * kc + h, hbd);
                wu = tf_weight_zz(be, a.decay[1]), wv = tf_weight_zz(be, a.decay[2]);
            }
        } else {
            uint32_t be[2], df[2], lw[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int q = 2 * k + h;
                be[k]       = tf_block_error(b, idx, q, hbd);
                df[k]       = split ? tf_d_factor(b.mv16_x[idx * 4 + q], b.mv16_y[idx * 4 + q], a.thr_shr8)
                                    : tf_d_factor(b.mv32_x[idx], b.mv32_y[idx], a.thr_shr8);
                uint32_t s = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int d = (int)cen_y[k][i] - (int)py[k][i];
                    s += (uint32_t)(d * d);
                }
                s = xor_add(s, 1), s = xor_add(s, 4), s = xor_add(s, 8), s = xor_add(s, 16), s = xor_add(s, 32);
                lw[k] = tf_window_error(s, 16, 16, shift);
                wy[k] = tf_weight(lw[k], be[k], df[k], split ? a.decay[0] : a.decay[0] << 1);
            }
            if (chroma) {
                uint32_t su = 0, sv = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int du = (int)cen_u[i] - (int)pu[i], dv = (int)cen_v[i] - (int)pv[i];
                    su += (uint32_t)(du * du), sv += (uint32_t)(dv * dv);
                }
                su = xor_add(su, 1), su = xor_add(su, 4), su = xor_add(su, 8), su = xor_add(su, 16);
                sv = xor_add(sv, 1), sv = xor_add(sv, 4), sv = xor_add(sv, 8), sv = xor_add(sv, 16);
                const uint32_t lwq = kc ? lw[1] : lw[0], beq = kc ? be[1] : be[0], dfq = kc ? df[1] : df[0];
                const uint32_t eu = (tf_window_error(su, 8, 8, shift) * 5u + lwq) / 6u;
                const uint32_t ev = (tf_window_error(sv, 8, 8, shift) * 5u + lwq) / 6u;
                wu = tf_weight(eu, beq, dfq, split ? a.decay[1] : a.decay[1] << 1);
                wv = tf_weight(ev, beq, dfq, split ? a.decay[2] : a.decay[2] << 1);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            cnt_y[k] += wy[k];
#pragma unroll
            for (int i = 0; i < 8; i++) acc_y[k][i] += wy[k] * py[k][i];
        }
        cnt_u += wu, cnt_v += wv;
#pragma unroll
        for (int i = 0; i < 4; i++) acc_u[i] += wu * pu[i], acc_v[i] += wv * pv[i];
    }

    // get_final_filtered_pixels: (accum + count / 2) / count
    T *oy = (T *)a.out[0];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        uint32_t o[8];
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = (acc_y[k][i] + (cnt_y[k] >> 1)) / cnt_y[k];
        pack_y(o, (typename Raw<T>::Y *)(oy + (size_t)(ly0 + 16 * k) * a.ostride[0] + lx));
    }
    uint32_t ou[4], ov[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ou[i] = chroma ? (acc_u[i] + (cnt_u >> 1)) / cnt_u : cen_u[i];
        ov[i] = chroma ? (acc_v[i] + (cnt_v >> 1)) / cnt_v : cen_v[i];
    }
    pack_c(ou, (typename Raw<T>::C *)((T *)a.out[1] + (size_t)cy * a.ostride[1] + cx));
    pack_c(ov, (typename Raw<T>::C *)((T *)a.out[2] + (size_t)cy * a.ostride[2] + cx));
}

// ---------------------------------------------------------------------------------------------
// the noise estimate
// ---------------------------------------------------------------------------------------------
struct NoiseSlot {
    unsigned long long sum, num;
    uint32_t           ticket;
    int32_t            result;
};
constexpr int kNoiseRows = 8; // rows of one wave; a workgroup covers 64 columns x 32 rows of the interior

template <typename T>
__global__ __launch_bounds__(256) void tf_noise_kernel(const T *src, int stride, int w, int h, int sh, NoiseSlot *slot) {
    __shared__ uint32_t part[4][2];
    const int           lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int           x = 1 + blockIdx.x * 64 + lane, y0 = 1 + (blockIdx.y * 4 + wave) * kNoiseRows;
    uint32_t            sum = 0, num = 0;
    const int           rnd = (1 << sh) >> 1;
    if (x < w - 1) {
        for (int y = y0; y < y0 + kNoiseRows && y < h - 1; y++) {
            const T  *p = src + (size_t)y * stride + x;
            const int a = p[-stride - 1], b = p[-stride], c = p[-stride + 1], d = p[-1], e = p[0], f = p[1];
            const int g = p[stride - 1], hh = p[stride], i = p[stride + 1];
            const int gx = (a - c) + (g - i) + 2 * (d - f), gy = (a - g) + (c - i) + 2 * (b - hh);
            const int ga = (abs(gx) + abs(gy) + rnd) >> sh;
            if (ga < 50) { // EDGE_THRESHOLD
                const int v = 4 * e - 2 * (d + f + b + hh) + (a + c + g + i);
                sum += (uint32_t)((abs(v) + rnd) >> sh);
                ++num;
            }
        }
    }
    sum = wave_total(sum), num = wave_total(num); // at most 64 * 8 * 16 * 65535: fits 32 bits
    if (lane == 0) part[wave][0] = sum, part[wave][1] = num;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = (unsigned long long)part[0][0] + part[1][0] + part[2][0] + part[3][0];
        const unsigned long long n = (unsigned long long)part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (s) atomicAdd(&slot->sum, s);
        if (n) atomicAdd(&slot->num, n);
        __threadfence();
        const uint32_t nblocks = gridDim.x * gridDim.y;
        if (atomicAdd(&slot->ticket, 1u) == nblocks - 1) { // the last workgroup: every sum has landed
            __threadfence();
            const long long ts = (long long)atomicAdd(&slot->sum, 0ull), tn = (long long)atomicAdd(&slot->num, 0ull);
            slot->result = tn < 16 ? -65536 : (int32_t)((ts * 82137) / (6 * tn)); // SMOOTH_THRESHOLD, SQRT_PI_BY_2_FP16
            slot->sum = 0, slot->num = 0, slot->ticket = 0; // ready for the next launch in stream order
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the shims' kernels: packed 16-bit samples, one launch each
// ---------------------------------------------------------------------------------------------
struct TfPlanePack { // byte offsets into the staging buffer of one plane's arrays, [h][w] each
    uint32_t src, pre, accum, count;
    int32_t  w, h;
};
struct TfBlockArgs {
    uint8_t      *buf;
    TfPlanePack   p[3];
    SvtGpuTfBlock blk;
    int32_t       idx, nplanes, bd, zz;
    uint32_t      decay[3], thr_shr8;
};
// one workgroup of four waves: wave q is quadrant q of every plane
__global__ __launch_bounds__(256) void tf_block_kernel(const TfBlockArgs a) {
    const int  lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool hbd = a.bd > 8, split = a.blk.split32[a.idx] != 0;
    const uint32_t be = tf_block_error(a.blk, a.idx, q, hbd);
    const uint32_t df = split ? tf_d_factor(a.blk.mv16_x[a.idx * 4 + q], a.blk.mv16_y[a.idx * 4 + q], a.thr_shr8)
                              : tf_d_factor(a.blk.mv32_x[a.idx], a.blk.mv32_y[a.idx], a.thr_shr8);
    uint32_t luma_win = 0;
    for (int p = 0; p < a.nplanes; p++) {
        const TfPlanePack &k  = a.p[p];
        const int          hw = k.w >> 1, hh = k.h >> 1, n = hw * hh, x0 = (q & 1) * hw, y0 = (q >> 1) * hh;
        const uint16_t    *src = (const uint16_t *)(a.buf + k.src), *pre = (const uint16_t *)(a.buf + k.pre);
        uint32_t          *acc = (uint32_t *)(a.buf + k.accum);
        uint16_t          *cnt = (uint16_t *)(a.buf + k.count);
        uint32_t           wgt;
        if (a.zz) {
            wgt = tf_weight_zz(be, a.decay[p]);
        } else {
            uint32_t s = 0;
            for (int i = lane; i < n; i += 64) {
                const int o = (y0 + i / hw) * k.w + x0 + i % hw, d = (int)src[o] - (int)pre[o];
                s += (uint32_t)(d * d);
            }
            uint32_t win = tf_window_error(wave_total(s), (uint32_t)hw, (uint32_t)hh, 2 * (a.bd - 8));
            if (p == 0)
                luma_win = win;
            else
                win = (win * 5u + luma_win) / 6u;
            wgt = tf_weight(win, be, df, split ? a.decay[p] : a.decay[p] << 1);
        }
        for (int i = lane; i < n; i += 64) {
            const int o = (y0 + i / hw) * k.w + x0 + i % hw;
            cnt[o]      = (uint16_t)(cnt[o] + wgt);
            acc[o] += wgt * pre[o];
        }
    }
}

// apply_filtering_central: n samples of packed src -> accum, count
__global__ void tf_central_kernel(const uint16_t *src, uint32_t *accum, uint16_t *count, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) accum[i] = kTfWeight * src[i], count[i] = (uint16_t)kTfWeight;
}
// get_final_filtered_pixels: n samples
__global__ void tf_final_kernel(const uint32_t *accum, const uint16_t *count, uint16_t *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t c = count[i];
        out[i]           = c ? (uint16_t)((accum[i] + (c >> 1)) / c) : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool bits_ok(int bits) { return bits == 8 || bits == 10; }

int launch_noise(const void *plane, int bits, int stride, int w, int h, NoiseSlot *slot, hipStream_t st) {
    const dim3 grid((unsigned)((w > 2 ? w - 2 : 1) + 63) / 64, (unsigned)((h > 2 ? h - 2 : 1) + 4 * kNoiseRows - 1) / (4 * kNoiseRows));
    if (bits == 8)
        hipLaunchKernelGGL(tf_noise_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t *)plane, stride, w, h, 0, slot);
    else
        hipLaunchKernelGGL(tf_noise_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t *)plane, stride, w, h, bits - 8,
                           slot);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}
bool noise_args_ok(const void *plane, int bits, int stride, int w, int h) {
    return plane && bits_ok(bits) && w > 0 && h > 0 && stride >= w && w <= 65536 && h <= 65536;
}

// The noise shim's slot stays apart from the thread's stage (svtgpu_stage_reserve): tf_noise_kernel resets sum / num /
// ticket itself and counts on finding them so at the next launch, so the slot's content must survive between calls,
// which a carved region of the growable buffer does not promise; the frame-level svtgpu_tf_estimate_noise uses it too, on
// a caller's stream.  One small allocation per thread, freed with it.
struct ThreadNoiseSlot {
    NoiseSlot *slot = nullptr;
    ~ThreadNoiseSlot() {
        if (slot) (void)hipFree(slot);
    }
};
thread_local ThreadNoiseSlot t_noise;
NoiseSlot *thread_noise_slot() {
    if (!t_noise.slot) {
        HIP_OR_DIE(hipMalloc(&t_noise.slot, sizeof(NoiseSlot)));
        HIP_OR_DIE(hipMemset(t_noise.slot, 0, sizeof(NoiseSlot)));
    }
    return t_noise.slot;
}

template <typename T>
int32_t shim_noise(const T *src, int w, int h, int stride, int bits) {
    if (!src || w <= 0 || h <= 0 || stride < w) svtgpu_fatal("svtgpu noise shim: bad arguments");
    hipStream_t  st = svtgpu_shim_stream();
    const size_t ds = ((size_t)w + 15) & ~(size_t)15, bytes = ds * h * sizeof(T);
    const SvtGpuStageLease sg = svtgpu_stage_reserve(bytes, st);
    uint8_t     *d  = sg.d;
    NoiseSlot   *sl = thread_noise_slot();
    HIP_OR_DIE(hipMemcpy2DAsync(d, ds * sizeof(T), src, (size_t)stride * sizeof(T), (size_t)w * sizeof(T), h,
                                hipMemcpyHostToDevice, st));
    if (launch_noise(d, bits, (int)ds, w, h, sl, st)) svtgpu_fatal("svtgpu noise shim: the launch failed");
    int32_t r = 0;
    HIP_OR_DIE(hipMemcpyAsync(&r, &sl->result, sizeof r, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    return r;
}

// packs [h][w] samples of a strided host plane as uint16
template <typename T> void pack_plane(uint16_t *dst, const T *src, int stride, int w, int h) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) dst[y * w + x] = src[(size_t)y * stride + x];
}

template <typename T>
void shim_block(const SvtGpuTfBlock *blk, int idx, const SvtGpuTfParams *prm, int zz, int bd, const T *const src[3],
                const int src_stride[3], const T *const pre[3], const int pre_stride[3], unsigned bw, unsigned bh, int ss_x,
                int ss_y, uint32_t *const accum[3], uint16_t *const count[3]) {
    if (!blk || !prm || idx < 0 || idx > 3 || bw < 2 || bh < 2 || bw > 64 || bh > 64 || (bw & 1) || (bh & 1) || !pre[0] ||
        !accum[0] || !count[0] || (!zz && !src[0]))
        svtgpu_fatal("svtgpu temporal filter shim: bad arguments");
    TfBlockArgs a;
    a.blk = *blk, a.idx = idx, a.nplanes = prm->tf_chroma ? 3 : 1, a.bd = bd, a.zz = zz;
    memcpy(a.decay, prm->decay_factor_fp16, sizeof a.decay);
    a.thr_shr8 = tf_threshold_shr8(prm->mv_dist_th);
    Carver c;
    for (int p = 0; p < a.nplanes; p++) {
        const int w = p ? (int)bw >> ss_x : (int)bw, h = p ? (int)bh >> ss_y : (int)bh;
        if (p && (!pre[p] || !accum[p] || !count[p] || (!zz && !src[p]))) svtgpu_fatal("svtgpu temporal filter shim: bad arguments");
        const size_t n = (size_t)w * h;
        a.p[p].w = w, a.p[p].h = h;
        a.p[p].accum = (uint32_t)c(4 * n), a.p[p].src = (uint32_t)c(2 * n), a.p[p].pre = (uint32_t)c(2 * n);
        a.p[p].count = (uint32_t)c(2 * n);
    }
    const size_t off = c.off;
    hipStream_t  st  = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(off, st);
    a.buf        = sg.d;
    uint8_t *hb  = sg.h;
    for (int p = 0; p < a.nplanes; p++) { // accum / count live with the predictor's stride (:1110)
        const TfPlanePack &k = a.p[p];
        if (!zz) pack_plane((uint16_t *)(hb + k.src), src[p], src_stride[p], k.w, k.h);
        pack_plane((uint16_t *)(hb + k.pre), pre[p], pre_stride[p], k.w, k.h);
        for (int y = 0; y < k.h; y++)
            for (int x = 0; x < k.w; x++) {
                ((uint32_t *)(hb + k.accum))[y * k.w + x] = accum[p][(size_t)y * pre_stride[p] + x];
                ((uint16_t *)(hb + k.count))[y * k.w + x] = count[p][(size_t)y * pre_stride[p] + x];
            }
    }
    HIP_OR_DIE(hipMemcpyAsync(a.buf, hb, off, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tf_block_kernel, dim3(1), dim3(256), 0, st, a);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(hb, a.buf, off, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    for (int p = 0; p < a.nplanes; p++) {
        const TfPlanePack &k = a.p[p];
        for (int y = 0; y < k.h; y++)
            for (int x = 0; x < k.w; x++) {
                accum[p][(size_t)y * pre_stride[p] + x] = ((const uint32_t *)(hb + k.accum))[y * k.w + x];
                count[p][(size_t)y * pre_stride[p] + x] = ((const uint16_t *)(hb + k.count))[y * k.w + x];
            }
    }
}

template <typename T>
void shim_central(int tf_chroma, int stride_y, T *const *src, uint32_t **accum, uint16_t **count, int bw, int bh, int ss_x,
                  int ss_y) {
    if (!src || !accum || !count || bw <= 0 || bh <= 0 || bw * bh > 4096 || stride_y < bw)
        svtgpu_fatal("svtgpu temporal filter shim: bad arguments");
    const int   np = tf_chroma ? 3 : 1;
    int         w[3], h[3], st_[3], n[3], tot = 0;
    for (int p = 0; p < np; p++) {
        w[p] = p ? bw >> ss_x : bw, h[p] = p ? bh >> ss_y : bh, st_[p] = p ? stride_y >> ss_x : stride_y;
        n[p] = w[p] * h[p], tot += n[p];
        if (!src[p] || !accum[p] || !count[p]) svtgpu_fatal("svtgpu temporal filter shim: bad arguments");
    }
    // device layout: accum u32 [tot], src u16 [tot], count u16 [tot]
    hipStream_t st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve((size_t)tot * 8, st);
    uint8_t *const d = sg.d, *const hb = sg.h;
    uint16_t   *hs = (uint16_t *)(hb + (size_t)tot * 4);
    for (int p = 0, o = 0; p < np; o += n[p], p++) pack_plane(hs + o, src[p], st_[p], w[p], h[p]);
    HIP_OR_DIE(hipMemcpyAsync(d + (size_t)tot * 4, hs, (size_t)tot * 2, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tf_central_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, (const uint16_t *)(d + (size_t)tot * 4),
                       (uint32_t *)d, (uint16_t *)(d + (size_t)tot * 6), tot);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(hb, d, (size_t)tot * 8, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    for (int p = 0, o = 0; p < np; o += n[p], p++) {
        memcpy(accum[p], (const uint32_t *)hb + o, (size_t)n[p] * 4);
        memcpy(count[p], (const uint16_t *)(hb + (size_t)tot * 6) + o, (size_t)n[p] * 2);
    }
}

} // namespace

struct SvtGpuTfState {
    SvtGpuContext *ctx;
    int32_t        width, height, blk_cols, nblk;
    NoiseSlot     *d_noise;
    uint8_t       *d_meta, *h_meta; // the filter: [n_refs] TfRef, then [n_refs][nblk] SvtGpuTfBlock; h_meta pinned
    size_t         cap_meta;        // bytes of each
    hipEvent_t     copied;          // the last upload of h_meta has left it
    hipStream_t    last;            // the stream of the last filter call
    uint8_t       *d_records;       // the search's records: [refs][nblk] SvtGpuTfMotion, then [refs][nblk] SvtGpuTfBlock
    int32_t        cap_records;     // in references; only grows
    int32_t        search_refs;     // the references of the last search
    uint8_t       *d_mask;          // the masked compound's DIFFWTD luma masks: width x height bytes, allocated on first use
};

namespace {
size_t meta_bytes(const SvtGpuTfState *s, int refs) { return (size_t)refs * (sizeof(TfRef) + (size_t)s->nblk * sizeof(SvtGpuTfBlock)); }

int meta_reserve(SvtGpuTfState *s, size_t bytes) {
    if (bytes <= s->cap_meta) return SVTGPU_OK;
    if (s->d_meta) { // an earlier call may still read it
        HIP_TRY(hipStreamSynchronize(s->last));
        (void)hipFree(s->d_meta), (void)hipHostFree(s->h_meta);
        s->d_meta = s->h_meta = nullptr, s->cap_meta = 0;
    }
    if (hipMalloc(&s->d_meta, bytes) != hipSuccess) return SVTGPU_ERR_OOM;
    if (hipHostMalloc(&s->h_meta, bytes) != hipSuccess) {
        (void)hipFree(s->d_meta);
        s->d_meta = nullptr;
        return SVTGPU_ERR_OOM;
    }
    s->cap_meta = bytes;
    return SVTGPU_OK;
}

bool planes_ok(const SvtGpuTfPlanes *p, int aw, int bs) {
    if (!p) return false;
    for (int k = 0; k < 3; k++) {
        const int need = aw >> (k > 0);
        if (!p->plane[k] || p->stride[k] < need || (((size_t)p->stride[k] * bs) & 15) || ((uintptr_t)p->plane[k] & 15)) return false;
    }
    return true;
}

// tf_frame_kernel on `a`, whose refs / blocks already point at device memory
int launch_frame(SvtGpuTfState *s, TfFrameArgs &a, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *out,
                 const SvtGpuTfParams *params, int n_refs, hipStream_t st) {
    for (int p = 0; p < 3; p++) {
        a.centre[p] = centre->plane[p], a.cstride[p] = centre->stride[p];
        a.out[p] = out->plane[p], a.ostride[p] = out->stride[p];
        a.decay[p] = params->decay_factor_fp16[p];
    }
    a.n_refs = n_refs, a.blk_cols = s->blk_cols, a.nblk = s->nblk;
    a.thr_shr8 = tf_threshold_shr8(params->mv_dist_th);
    a.tf_chroma = params->tf_chroma, a.bd = params->bit_depth, a.zz = params->use_zz_based_filter;
    s->last = st;
    if (params->bit_depth == 8)
        hipLaunchKernelGGL(tf_frame_kernel<uint8_t>, dim3(s->nblk), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(tf_frame_kernel<uint16_t>, dim3(s->nblk), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}
} // namespace

// The state's metadata buffer for svtgpu_tf_predict_frame (interp.hip), under the filter's rule: one pinned host copy,
// rewritten once the previous upload has left it, and a device copy that the calls of one stream reuse in order.
void svtgpu_tf_state_geometry(const SvtGpuTfState *s, SvtGpuContext **ctx, int32_t *width, int32_t *height,
                              int32_t *blk_cols, int32_t *nblk) {
    *ctx = s->ctx, *width = s->width, *height = s->height, *blk_cols = s->blk_cols, *nblk = s->nblk;
}
int svtgpu_tf_meta_begin(SvtGpuTfState *s, size_t bytes, uint8_t **host, uint8_t **dev) {
    if (int rc = meta_reserve(s, bytes)) return rc;
    HIP_TRY(hipEventSynchronize(s->copied));
    *host = s->h_meta, *dev = s->d_meta;
    return SVTGPU_OK;
}
int svtgpu_tf_meta_upload(SvtGpuTfState *s, size_t bytes, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(s->d_meta, s->h_meta, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->copied, st));
    svtgpu_count_xfer(0, bytes);
    s->last = st;
    return SVTGPU_OK;
}

// The search's record buffer (tf_search.hip writes it, svtgpu_tf_compensate_filter_frame reads it): grown for n_refs, never
// shrunk; growing waits for the work queued on the state, which may still read the old buffer.
int svtgpu_tf_records_reserve(SvtGpuTfState *s, int n_refs, SvtGpuTfMotion **motion, SvtGpuTfBlock **blocks) {
    if (n_refs > s->cap_records) {
        if (s->d_records) {
            HIP_TRY(hipStreamSynchronize(s->last));
            (void)hipFree(s->d_records);
            s->d_records = nullptr, s->cap_records = 0;
        }
        if (hipMalloc(&s->d_records, (size_t)n_refs * s->nblk * (sizeof(SvtGpuTfMotion) + sizeof(SvtGpuTfBlock))) != hipSuccess)
            return SVTGPU_ERR_OOM;
        s->cap_records = n_refs;
    }
    *motion = (SvtGpuTfMotion *)s->d_records;
    *blocks = (SvtGpuTfBlock *)(s->d_records + (size_t)n_refs * s->nblk * sizeof(SvtGpuTfMotion));
    return SVTGPU_OK;
}
// The DIFFWTD mask plane of svtgpu_masked_compound_predict_batch (masked_compound.hip): one byte per luma sample of the
// state's picture, stride width.  Allocated once, so no call queued on the state ever sees it move.
int svtgpu_tf_mask_reserve(SvtGpuTfState *s, uint8_t **mask) {
    if (!s->d_mask && hipMalloc(&s->d_mask, (size_t)s->width * s->height) != hipSuccess) {
        s->d_mask = nullptr;
        return SVTGPU_ERR_OOM;
    }
    *mask = s->d_mask;
    return SVTGPU_OK;
}
void svtgpu_tf_records_commit(SvtGpuTfState *s, int n_refs) { s->search_refs = n_refs; }
int  svtgpu_tf_records_get(SvtGpuTfState *s, SvtGpuTfMotion **motion, SvtGpuTfBlock **blocks) {
    *motion = (SvtGpuTfMotion *)s->d_records;
    *blocks = (SvtGpuTfBlock *)(s->d_records + (size_t)s->search_refs * s->nblk * sizeof(SvtGpuTfMotion));
    return s->search_refs;
}

// ---------------------------------------------------------------------------------------------
// host-only entry points
// ---------------------------------------------------------------------------------------------
extern "C" int32_t svtgpu_tf_noise_log1p_fp16(int32_t noise_level_fp16) { // svt_aom_noise_log1p_fp16 (:656-675)
    const int64_t base = 65536 + (int64_t)noise_level_fp16;
    if (base <= 0) return INT32_MIN;
    if (base < 458752) {
        const int     id   = (int)(base >> 11);
        const int64_t rest = base & 0x7FF;
        return (int32_t)(kTfLog1pFp16[id] + ((rest * ((int64_t)kTfLog1pFp16[id + 1] - kTfLog1pFp16[id])) >> 11));
    }
    return ((1860 * (noise_level_fp16 >> 8)) >> 8) + 116456;
}

extern "C" uint32_t svtgpu_tf_decay_factor_fp16(int32_t decay_control, int32_t noise_log1p_fp16, int32_t q) { // :2913-2927
    const uint32_t q_decay_fp8  = q >= 128 ? (uint32_t)(q * q) >> 5 : (uint32_t)((q << 2) > 1 ? (q << 2) : 1);
    const int32_t  n_decay_fp10 = (int32_t)(((int64_t)decay_control * (45875 + (int64_t)noise_log1p_fp16)) / 64);
    return (uint32_t)((((int64_t)n_decay_fp10 * (int64_t)n_decay_fp10) * q_decay_fp8) >> 11);
}

extern "C" int svtgpu_tf_tables(const int32_t **log1p_fp16, int32_t *n_log1p, const uint32_t **sqrt_fp16,
                                const int32_t **expf_fp16, int32_t *n_expf) {
    if (!log1p_fp16 || !n_log1p || !sqrt_fp16 || !expf_fp16 || !n_expf) return SVTGPU_ERR_INVALID_ARG;
    *log1p_fp16 = kTfLog1pFp16, *n_log1p = (int32_t)(sizeof kTfLog1pFp16 / sizeof kTfLog1pFp16[0]);
    *sqrt_fp16 = kTfSqrtFp16;
    *expf_fp16 = kTfExpfFp16, *n_expf = (int32_t)(sizeof kTfExpfFp16 / sizeof kTfExpfFp16[0]);
    return SVTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// device entry points
// ---------------------------------------------------------------------------------------------
extern "C" int svtgpu_tf_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, SvtGpuTfState **out) {
    if (!ctx || !out || width <= 0 || height <= 0 || (width & 7) || (height & 7) || width > 65536 || height > 65536)
        return SVTGPU_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    SvtGpuTfState *s = new SvtGpuTfState();
    s->ctx = ctx, s->width = width, s->height = height;
    s->blk_cols = (width + 63) / 64, s->nblk = s->blk_cols * ((height + 63) / 64);
    s->last = ctx->stream;
    if (hipMalloc(&s->d_noise, sizeof(NoiseSlot)) != hipSuccess || hipMemset(s->d_noise, 0, sizeof(NoiseSlot)) != hipSuccess ||
        hipEventCreateWithFlags(&s->copied, hipEventDisableTiming) != hipSuccess) {
        if (s->d_noise) (void)hipFree(s->d_noise);
        delete s;
        return SVTGPU_ERR_OOM;
    }
    *out = s;
    return SVTGPU_OK;
}

extern "C" void svtgpu_tf_state_destroy(SvtGpuTfState *s) {
    if (!s) return;
    (void)hipStreamSynchronize(s->last);
    (void)hipEventDestroy(s->copied);
    if (s->d_meta) (void)hipFree(s->d_meta);
    if (s->h_meta) (void)hipHostFree(s->h_meta);
    if (s->d_records) (void)hipFree(s->d_records);
    if (s->d_mask) (void)hipFree(s->d_mask);
    (void)hipFree(s->d_noise);
    delete s;
}

extern "C" int svtgpu_tf_estimate_noise(SvtGpuContext *ctx, const void *plane, int32_t bits, int32_t stride, int32_t w,
                                        int32_t h, void *stream, int32_t *out_fp16) {
    if (!ctx || !out_fp16 || !noise_args_ok(plane, bits, stride, w, h)) return SVTGPU_ERR_INVALID_ARG;
    hipStream_t st = pick_stream(ctx, stream);
    NoiseSlot  *sl = thread_noise_slot();
    if (int rc = launch_noise(plane, bits, stride, w, h, sl, st)) return rc;
    HIP_TRY(hipMemcpyAsync(out_fp16, &sl->result, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SVTGPU_OK;
}

extern "C" int svtgpu_tf_estimate_noise_async(SvtGpuTfState *s, const void *plane, int32_t bits, int32_t stride, int32_t w,
                                              int32_t h, void *stream) {
    if (!s || !noise_args_ok(plane, bits, stride, w, h)) return SVTGPU_ERR_INVALID_ARG;
    return launch_noise(plane, bits, stride, w, h, s->d_noise, pick_stream(s->ctx, stream));
}

extern "C" int svtgpu_tf_read_noise(SvtGpuTfState *s, void *stream, int32_t *out_fp16) {
    if (!s || !out_fp16) return SVTGPU_ERR_INVALID_ARG;
    hipStream_t st = pick_stream(s->ctx, stream);
    HIP_TRY(hipMemcpyAsync(out_fp16, &s->d_noise->result, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SVTGPU_OK;
}

extern "C" int svtgpu_tf_filter_frame(SvtGpuTfState *s, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs,
                                      int32_t n_refs, const SvtGpuTfBlock *blocks, const SvtGpuTfParams *params,
                                      const SvtGpuTfPlanes *out, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED; // count is 16 bits in the reference: 27 x 1000 is its limit
    if (!s || !params || n_refs < 0 || (n_refs && (!refs || !blocks)) || !bits_ok(params->bit_depth))
        return SVTGPU_ERR_INVALID_ARG;
    const int bs = params->bit_depth > 8 ? 2 : 1, aw = s->blk_cols * 64;
    if (!planes_ok(centre, aw, bs) || !planes_ok(out, aw, bs)) return SVTGPU_ERR_INVALID_ARG;
    for (int r = 0; r < n_refs; r++)
        if (!planes_ok(&refs[r], aw, bs)) return SVTGPU_ERR_INVALID_ARG;
    hipStream_t st = pick_stream(s->ctx, stream);
    TfFrameArgs a;
    memset(&a, 0, sizeof a);
    if (n_refs) {
        if (int rc = meta_reserve(s, meta_bytes(s, n_refs))) return rc;
        HIP_TRY(hipEventSynchronize(s->copied)); // the previous call's upload has left the pinned buffer
        TfRef *hr = (TfRef *)s->h_meta;
        for (int r = 0; r < n_refs; r++)
            for (int p = 0; p < 3; p++) hr[r].plane[p] = refs[r].plane[p], hr[r].stride[p] = refs[r].stride[p];
        const size_t off = (size_t)n_refs * sizeof(TfRef), nb = (size_t)n_refs * s->nblk * sizeof(SvtGpuTfBlock);
        memcpy(s->h_meta + off, blocks, nb);
        HIP_TRY(hipMemcpyAsync(s->d_meta, s->h_meta, off + nb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(s->copied, st));
        svtgpu_count_xfer(0, off + nb);
        a.refs = (const TfRef *)s->d_meta, a.blocks = (const SvtGpuTfBlock *)(s->d_meta + off);
    }
    return launch_frame(s, a, centre, out, params, n_refs, st);
}

// The device chain after svtgpu_tf_search_frame: the compensation on the state's motion records, err32 of the use64
// blocks, the filter on the state's block records.  One small upload of plane descriptors; no record leaves the device.
extern "C" int svtgpu_tf_compensate_filter_frame(SvtGpuTfState *s, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs,
                                                 int32_t n_refs, int32_t border_x, int32_t border_y,
                                                 const SvtGpuTfParams *params, int32_t sub_sampling_shift,
                                                 const SvtGpuTfPlanes *pred, const SvtGpuTfPlanes *out, void *stream) {
    if (n_refs > kMaxRefs) return SVTGPU_ERR_UNSUPPORTED;
    if (!s || !params || n_refs < 0 || (n_refs && (!refs || !pred)) || !bits_ok(params->bit_depth) || border_x < 0 ||
        border_y < 0 || (sub_sampling_shift != 0 && sub_sampling_shift != 1) || n_refs != s->search_refs)
        return SVTGPU_ERR_INVALID_ARG;
    const int bs = params->bit_depth > 8 ? 2 : 1, aw = s->blk_cols * 64, nplanes = params->tf_chroma ? 3 : 1;
    if (!planes_ok(centre, aw, bs) || !planes_ok(out, aw, bs)) return SVTGPU_ERR_INVALID_ARG;
    for (int r = 0; r < n_refs; r++) {
        if (!planes_ok(&pred[r], aw, bs)) return SVTGPU_ERR_INVALID_ARG; // the filter reads all three predictor planes
        for (int p = 0; p < nplanes; p++) {
            const int ss = p > 0;
            if (!refs[r].plane[p] || ((uintptr_t)refs[r].plane[p] & (bs - 1)) ||
                refs[r].stride[p] < (s->width >> ss) + 2 * (border_x >> ss))
                return SVTGPU_ERR_INVALID_ARG;
        }
    }
    hipStream_t st = pick_stream(s->ctx, stream);
    TfFrameArgs a;
    memset(&a, 0, sizeof a);
    if (n_refs) {
        const size_t o_ref = (size_t)n_refs * svtgpu_tf_predict_desc_bytes(), o_luma = o_ref + (size_t)n_refs * sizeof(TfRef);
        const size_t total = o_luma + (size_t)n_refs * sizeof(SvtGpuTfLuma);
        uint8_t     *hm, *dm;
        if (int rc = svtgpu_tf_meta_begin(s, total, &hm, &dm)) return rc;
        svtgpu_tf_predict_desc_fill(hm, refs, pred, n_refs);
        TfRef        *hr = (TfRef *)(hm + o_ref);
        SvtGpuTfLuma *hl = (SvtGpuTfLuma *)(hm + o_luma);
        for (int r = 0; r < n_refs; r++) {
            for (int p = 0; p < 3; p++) hr[r].plane[p] = pred[r].plane[p], hr[r].stride[p] = pred[r].stride[p];
            hr[r].pad = 0, hl[r].plane = pred[r].plane[0], hl[r].stride = pred[r].stride[0], hl[r].pad = 0;
        }
        if (int rc = svtgpu_tf_meta_upload(s, total, st)) return rc;
        SvtGpuTfMotion *dmo;
        SvtGpuTfBlock  *dbl;
        svtgpu_tf_records_get(s, &dmo, &dbl);
        if (int rc = svtgpu_tf_predict_launch(s, dm, dmo, n_refs, border_x, border_y, params->bit_depth, params->tf_chroma, st))
            return rc;
        if (int rc = svtgpu_tf_err64_launch(s, centre, (const SvtGpuTfLuma *)(dm + o_luma), dmo, dbl, n_refs, params->bit_depth,
                                            sub_sampling_shift, st))
            return rc;
        a.refs = (const TfRef *)(dm + o_ref), a.blocks = dbl;
    }
    return launch_frame(s, a, centre, out, params, n_refs, st);
}

// ---------------------------------------------------------------------------------------------
// RTCD shims: host pointers, synchronous.  The two noise functions carry the reference's prototypes
// (aom_dsp_rtcd.h:874-877); the other seven are what svtgpu_rtcd.h's adapters call with the MeContext fields read out.
// ---------------------------------------------------------------------------------------------
extern "C" int32_t svtgpu_estimate_noise_fp16(const uint8_t *src, uint16_t width, uint16_t height, uint16_t stride_y) {
    return shim_noise<uint8_t>(src, width, height, stride_y, 8);
}
extern "C" int32_t svtgpu_estimate_noise_highbd_fp16(const uint16_t *src, int width, int height, int stride, int bd) {
    if (!bits_ok(bd)) svtgpu_fatal("svtgpu noise shim: bit depth other than 8 or 10");
    return shim_noise<uint16_t>(src, width, height, stride, bd);
}

extern "C" void svtgpu_tf_apply_planewise_medium(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                                 const uint8_t *y_src, int y_src_stride, const uint8_t *y_pre,
                                                 int y_pre_stride, const uint8_t *u_src, const uint8_t *v_src,
                                                 int uv_src_stride, const uint8_t *u_pre, const uint8_t *v_pre,
                                                 int uv_pre_stride, unsigned int block_width, unsigned int block_height,
                                                 int ss_x, int ss_y, uint32_t *y_accum, uint16_t *y_count,
                                                 uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count) {
    const uint8_t *const src[3] = {y_src, u_src, v_src}, *const pre[3] = {y_pre, u_pre, v_pre};
    const int            ss[3] = {y_src_stride, uv_src_stride, uv_src_stride}, ps[3] = {y_pre_stride, uv_pre_stride, uv_pre_stride};
    uint32_t *const      acc[3] = {y_accum, u_accum, v_accum};
    uint16_t *const      cnt[3] = {y_count, u_count, v_count};
    shim_block<uint8_t>(blk, idx_32x32, prm, 0, 8, src, ss, pre, ps, block_width, block_height, ss_x, ss_y, acc, cnt);
}
extern "C" void svtgpu_tf_apply_planewise_medium_hbd(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                                     const uint16_t *y_src, int y_src_stride, const uint16_t *y_pre,
                                                     int y_pre_stride, const uint16_t *u_src, const uint16_t *v_src,
                                                     int uv_src_stride, const uint16_t *u_pre, const uint16_t *v_pre,
                                                     int uv_pre_stride, unsigned int block_width, unsigned int block_height,
                                                     int ss_x, int ss_y, uint32_t *y_accum, uint16_t *y_count,
                                                     uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum,
                                                     uint16_t *v_count, uint32_t encoder_bit_depth) {
    const uint16_t *const src[3] = {y_src, u_src, v_src}, *const pre[3] = {y_pre, u_pre, v_pre};
    const int             ss[3] = {y_src_stride, uv_src_stride, uv_src_stride}, ps[3] = {y_pre_stride, uv_pre_stride, uv_pre_stride};
    uint32_t *const       acc[3] = {y_accum, u_accum, v_accum};
    uint16_t *const       cnt[3] = {y_count, u_count, v_count};
    if (!bits_ok((int)encoder_bit_depth)) svtgpu_fatal("svtgpu temporal filter shim: bit depth other than 8 or 10");
    shim_block<uint16_t>(blk, idx_32x32, prm, 0, (int)encoder_bit_depth, src, ss, pre, ps, block_width, block_height, ss_x, ss_y,
                         acc, cnt);
}
extern "C" void svtgpu_tf_apply_zz_planewise_medium(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                                    const uint8_t *y_pre, int y_pre_stride, const uint8_t *u_pre,
                                                    const uint8_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                                    unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum,
                                                    uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                                    uint32_t *v_accum, uint16_t *v_count) {
    const uint8_t *const src[3] = {nullptr, nullptr, nullptr}, *const pre[3] = {y_pre, u_pre, v_pre};
    const int            ps[3] = {y_pre_stride, uv_pre_stride, uv_pre_stride};
    uint32_t *const      acc[3] = {y_accum, u_accum, v_accum};
    uint16_t *const      cnt[3] = {y_count, u_count, v_count};
    shim_block<uint8_t>(blk, idx_32x32, prm, 1, 8, src, ps, pre, ps, block_width, block_height, ss_x, ss_y, acc, cnt);
}
extern "C" void svtgpu_tf_apply_zz_planewise_medium_hbd(const SvtGpuTfBlock *blk, int32_t idx_32x32,
                                                        const SvtGpuTfParams *prm, const uint16_t *y_pre, int y_pre_stride,
                                                        const uint16_t *u_pre, const uint16_t *v_pre, int uv_pre_stride,
                                                        unsigned int block_width, unsigned int block_height, int ss_x,
                                                        int ss_y, uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum,
                                                        uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count,
                                                        uint32_t encoder_bit_depth) {
    const uint16_t *const src[3] = {nullptr, nullptr, nullptr}, *const pre[3] = {y_pre, u_pre, v_pre};
    const int             ps[3] = {y_pre_stride, uv_pre_stride, uv_pre_stride};
    uint32_t *const       acc[3] = {y_accum, u_accum, v_accum};
    uint16_t *const       cnt[3] = {y_count, u_count, v_count};
    if (!bits_ok((int)encoder_bit_depth)) svtgpu_fatal("svtgpu temporal filter shim: bit depth other than 8 or 10");
    shim_block<uint16_t>(blk, idx_32x32, prm, 1, (int)encoder_bit_depth, src, ps, pre, ps, block_width, block_height, ss_x, ss_y,
                         acc, cnt);
}

extern "C" void svtgpu_tf_apply_filtering_central(int32_t tf_chroma, int32_t src_stride_y, uint8_t **src, uint32_t **accum,
                                                  uint16_t **count, uint16_t blk_width, uint16_t blk_height, uint32_t ss_x,
                                                  uint32_t ss_y) {
    shim_central<uint8_t>(tf_chroma, src_stride_y, src, accum, count, blk_width, blk_height, (int)ss_x, (int)ss_y);
}
extern "C" void svtgpu_tf_apply_filtering_central_highbd(int32_t tf_chroma, int32_t src_stride_y, uint16_t **src_16bit,
                                                         uint32_t **accum, uint16_t **count, uint16_t blk_width,
                                                         uint16_t blk_height, uint32_t ss_x, uint32_t ss_y) {
    shim_central<uint16_t>(tf_chroma, src_stride_y, src_16bit, accum, count, blk_width, blk_height, (int)ss_x, (int)ss_y);
}

// get_final_filtered_pixels (:2582-2646): luma is 64x64, chroma blk_width_ch x blk_height_ch, accum / count packed
extern "C" void svtgpu_tf_get_final_filtered_pixels(int32_t tf_chroma, uint8_t **src_center_ptr_start,
                                                    uint16_t **altref_buffer_highbd_start, uint32_t **accum,
                                                    uint16_t **count, const uint32_t *stride, int blk_y_src_offset,
                                                    int blk_ch_src_offset, uint16_t blk_width_ch, uint16_t blk_height_ch,
                                                    int is_highbd) {
    if (!accum || !count || !stride || (is_highbd ? !altref_buffer_highbd_start : !src_center_ptr_start) ||
        (int)blk_width_ch * blk_height_ch > 4096)
        svtgpu_fatal("svtgpu temporal filter shim: bad arguments");
    const int np = tf_chroma ? 3 : 1;
    const int w[3] = {64, blk_width_ch, blk_width_ch}, h[3] = {64, blk_height_ch, blk_height_ch};
    int       n[3], tot = 0;
    for (int p = 0; p < np; p++) n[p] = w[p] * h[p], tot += n[p];
    // device layout: accum u32 [tot], count u16 [tot], out u16 [tot]
    hipStream_t st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve((size_t)tot * 8, st);
    uint8_t *const d = sg.d, *const hb = sg.h;
    for (int p = 0, o = 0; p < np; o += n[p], p++) {
        memcpy((uint32_t *)hb + o, accum[p], (size_t)n[p] * 4);
        memcpy((uint16_t *)(hb + (size_t)tot * 4) + o, count[p], (size_t)n[p] * 2);
    }
    HIP_OR_DIE(hipMemcpyAsync(d, hb, (size_t)tot * 6, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tf_final_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, (const uint32_t *)d,
                       (const uint16_t *)(d + (size_t)tot * 4), (uint16_t *)(d + (size_t)tot * 6), tot);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipMemcpyAsync(hb + (size_t)tot * 6, d + (size_t)tot * 6, (size_t)tot * 2, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    const uint16_t *res = (const uint16_t *)(hb + (size_t)tot * 6);
    for (int p = 0, o = 0; p < np; o += n[p], p++) {
        const size_t off = p ? (size_t)blk_ch_src_offset : (size_t)blk_y_src_offset;
        for (int y = 0; y < h[p]; y++)
            for (int x = 0; x < w[p]; x++) {
                const uint16_t v = res[o + y * w[p] + x];
                const size_t at = off + (size_t)y * stride[p ? 1 : 0] + x; // both chroma planes by stride[C_U] (:2617)
                if (is_highbd)
                    altref_buffer_highbd_start[p][at] = v;
                else
                    src_center_ptr_start[p][at] = (uint8_t)v;
            }
    }
}
