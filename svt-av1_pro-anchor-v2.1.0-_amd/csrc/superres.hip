// superres.hip — AV1 super-resolution: the normative horizontal upscale between CDEF and loop restoration on gfx950.
//
//   svt_av1_upscale_normative_rows (Source/Lib/Common/Codec/EbSuperRes.c:214-284) for one plane, as called per plane by
//   svt_av1_superres_upscale_frame (EbRestProcess.c:405-458) on the CDEF output and, two rows at a time, by
//   svt_aom_save_deblock_boundary_lines (EbRestoration.c:1544-1560) on the deblocked frame.
//
// Output column X of a plane samples source position x0_qn + X * x_step_qn (14 fractional bits): taps
// (x_qn >> 14) - 4 + k, k = 0..7, of row (x_qn & 0x3fff) >> 8 of the 64 x 8 filter table, rounded by 7 bits and clipped.
// The reference walks the tile columns, carries x0_qn across them and replicates only at the picture's edges, so the
// position of a column does not depend on the tile columns and this file takes none.  Source indices are clamped to
// [0, src_plane_width - 1]: the reference replicates from the last tile column's end (the coded width), and the
// columns between the crop and the coded width are read as they lie.
//
// A workgroup is 4 waves, one output row each, 512 outputs per row.  A wave reads the source window of its 512 outputs
// once, with 16-B loads on the aligned interior, into LDS as 16-bit samples; the filter table sits in LDS as 64 rows of
// 8 packed int16.  A lane then makes 8 adjacent outputs: it takes the 16 samples they can reach (the step is at most
// one source sample per output) from LDS into 8 registers, slides them by 0 or 1 sample per output with
// v_alignbyte_b32, runs the taps as 4 v_dot2c_i32_i16 and stores the 8 results at once.
#include "resize_tables.h" // kUpscaleFilter: av1_resize_filter_normative, shared with resize.hip
#include "svtgpu_internal.h"

namespace {

constexpr int kOutPerLane = 8;
constexpr int kTileW      = 64 * kOutPerLane; // outputs of one wave
constexpr int kRowsPerWg  = 4;
// samples of one wave's LDS window: the taps of kTileW outputs span at most kTileW + 8 source samples, the window
// starts up to 15 samples before them (16-B aligned loads of 8-bit samples), and a lane reads 16 samples from an even
// index at most 7 before the last tap's window start
constexpr int kWin = 560;

typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

struct UpscaleArgs {
    const void *src;
    void       *dst;
    int32_t     src_stride, dst_stride; // samples
    int32_t     src_w;                  // the source plane's coded width: indices are clamped to [0, src_w - 1]
    int32_t     out_w, dst_w;           // upscaled columns; columns written (the rest repeat column out_w - 1)
    int32_t     rows, x_step_qn, x0_qn, maxv;
    int32_t     aligned; // every source row starts 16-B aligned
};

template <typename T>
__global__ __launch_bounds__(64 * kRowsPerWg) void superres_upscale_kernel(const UpscaleArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T); // samples of one 16-B load
    __shared__ __attribute__((aligned(16))) uint16_t win[kRowsPerWg][kWin];
    __shared__ uint4 filt[64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.y * kRowsPerWg + wave, X0 = blockIdx.x * kTileW;
    if (threadIdx.x < 64) filt[threadIdx.x] = ((const uint4 *)kUpscaleFilter)[threadIdx.x];

    // the wave's source window [a0, a0 + n): first tap of its first output (rounded down to a 16-B load) .. last tap of
    // its last output
    const int last = a.out_w - 1;
    const int s_lo = ((a.x0_qn + min(X0, last) * a.x_step_qn) >> 14) - 4;
    const int s_hi = ((a.x0_qn + min(X0 + kTileW - 1, last) * a.x_step_qn) >> 14) + 3;
    const int a0   = s_lo & ~(VEC - 1); // floor to a multiple of VEC (two's complement, s_lo >= -4)
    const int n    = s_hi - a0 + 1;     // <= kTileW + 8 + VEC - 1
    if (y < a.rows) {
        const T  *row = (const T *)a.src + (size_t)y * a.src_stride;
        uint16_t *w   = win[wave];
        for (int c = lane * VEC; c < n; c += 64 * VEC) {
            const int b = a0 + c;
            if (a.aligned && b >= 0 && b + VEC <= a.src_w) {
                const uint4 v = *(const uint4 *)(row + b);
                if (sizeof(T) == 2) {
                    *(uint4 *)(w + c) = v;
                } else {
                    const uint32_t in[4] = {v.x, v.y, v.z, v.w};
                    uint32_t       o[8];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        o[2 * k]     = __builtin_amdgcn_perm(0u, in[k], 0x0c010c00u); // bytes 0,1 -> u16 lanes
                        o[2 * k + 1] = __builtin_amdgcn_perm(0u, in[k], 0x0c030c02u);
                    }
                    ((uint4 *)(w + c))[0] = make_uint4(o[0], o[1], o[2], o[3]);
                    ((uint4 *)(w + c))[1] = make_uint4(o[4], o[5], o[6], o[7]);
                }
            } else { // a picture edge or an unaligned row: one sample at a time, the index clamped
                for (int k = 0; k < VEC; k++) w[c + k] = (uint16_t)row[min(max(b + k, 0), a.src_w - 1)];
            }
        }
    }
    __syncthreads();

    const int X = X0 + lane * kOutPerLane;
    if (y >= a.rows || X >= a.dst_w) return;
    int xq = a.x0_qn + min(X, last) * a.x_step_qn;
    int s  = (xq >> 14) - 4;
    // 16 samples from the even index at or below the first tap; r[0] is then slid so the taps start at its low half
    const uint32_t *w32 = (const uint32_t *)win[wave] + ((s - a0) >> 1);
    uint32_t        r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = w32[k];
    uint32_t sh = (uint32_t)((s - a0) & 1) * 2; // bytes to slide by
    int      out[kOutPerLane];
#pragma unroll
    for (int j = 0; j < kOutPerLane; j++) {
#pragma unroll
        for (int k = 0; k < 7; k++) r[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], sh);
        r[7] >>= 8 * sh;
        const uint4 f   = filt[(xq & 0x3fff) >> 8];
        int         sum = dot2(r[0], f.x, 64);
        sum             = dot2(r[1], f.y, sum);
        sum             = dot2(r[2], f.z, sum);
        sum             = dot2(r[3], f.w, sum);
        out[j]          = min(max(sum >> 7, 0), a.maxv);
        // the next output: the same column again past out_w - 1 (the row's last upscaled sample repeats)
        const int xn = xq + (X + j < last ? a.x_step_qn : 0);
        sh           = (uint32_t)((xn >> 14) - (xq >> 14)) * 2; // 0 or 1 sample: x_step_qn <= 1 << 14
        xq           = xn;
    }
    T *d = (T *)a.dst + (size_t)y * a.dst_stride + X;
    if (X + kOutPerLane <= a.dst_w && !((uintptr_t)d & (kOutPerLane * sizeof(T) - 1))) {
        if (sizeof(T) == 2)
            *(uint4 *)d = make_uint4(out[0] | out[1] << 16, out[2] | out[3] << 16, out[4] | out[5] << 16,
                                     out[6] | out[7] << 16);
        else
            *(uint2 *)d = make_uint2(out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24,
                                     out[4] | out[5] << 8 | out[6] << 16 | out[7] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kOutPerLane; j++)
            if (X + j < a.dst_w) d[j] = (T)out[j];
    }
}

int upscale_dev(const void *src, int bits, int src_stride, int src_w, int in_w, void *dst, int dst_stride, int dst_w,
                int out_w, int rows, int bit_depth, hipStream_t st) {
    if (!src || !dst || src == dst || (bits != 8 && bits != 16) || rows <= 0 || in_w <= 0 || out_w < in_w ||
        out_w > 2 * in_w || out_w > 65536 || src_w < in_w || src_stride < src_w || dst_w < out_w || dst_stride < dst_w ||
        bit_depth < 8 || bit_depth > (bits == 8 ? 8 : 12))
        return SVTGPU_ERR_INVALID_ARG;
    UpscaleArgs a;
    a.src = src, a.dst = dst, a.src_stride = src_stride, a.dst_stride = dst_stride, a.src_w = src_w;
    a.out_w = out_w, a.dst_w = dst_w, a.rows = rows, a.maxv = (1 << bit_depth) - 1;
    if (int rc = svtgpu_superres_geometry(in_w, out_w, &a.x_step_qn, &a.x0_qn)) return rc;
    a.aligned = !(((uintptr_t)src | ((size_t)src_stride * (bits / 8))) & 15);
    const dim3 grid((dst_w + kTileW - 1) / kTileW, (rows + kRowsPerWg - 1) / kRowsPerWg);
    if (grid.y > 65535) return SVTGPU_ERR_INVALID_ARG;
    if (bits == 8)
        hipLaunchKernelGGL(superres_upscale_kernel<uint8_t>, grid, dim3(64 * kRowsPerWg), 0, st, a);
    else
        hipLaunchKernelGGL(superres_upscale_kernel<uint16_t>, grid, dim3(64 * kRowsPerWg), 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

} // namespace

// calculate_scaled_size_helper (EbSuperRes.c:22-41); host only
extern "C" int32_t svtgpu_superres_scaled_size(int32_t dim, int32_t denom) {
    if (denom != 8 && denom >= 1 && denom <= 16) {
        const int32_t min_dim = dim < 16 ? dim : 16;
        const int32_t d       = (dim * 8 + denom / 2) / denom;
        return d > min_dim ? d : min_dim;
    }
    if (denom == 17) return (3 + dim * 3) >> 2;
    return dim;
}

// av1_get_upscale_convolve_step / get_upscale_convolve_x0 (EbSuperRes.c:43-52); host only
extern "C" int svtgpu_superres_geometry(int32_t in_w, int32_t out_w, int32_t *x_step_qn, int32_t *x0_qn) {
    if (!x_step_qn || !x0_qn || in_w <= 0 || out_w <= 0 || in_w > 65536 || out_w > 65536) return SVTGPU_ERR_INVALID_ARG;
    const int32_t step = ((in_w << 14) + out_w / 2) / out_w;
    const int32_t err  = out_w * step - (in_w << 14);
    const int32_t x0   = (-((out_w - in_w) * (1 << 13)) + out_w / 2) / out_w + 128 - err / 2;
    *x_step_qn         = step;
    *x0_qn             = (int32_t)((uint32_t)x0 & 0x3fffu);
    return SVTGPU_OK;
}

extern "C" int svtgpu_superres_upscale_plane(const void *src, int32_t bits, int32_t src_stride, int32_t src_plane_width,
                                             int32_t in_w, void *dst, int32_t dst_stride, int32_t dst_plane_width,
                                             int32_t out_w, int32_t rows, int32_t bit_depth, void *stream) {
    return upscale_dev(src, bits, src_stride, src_plane_width, in_w, dst, dst_stride, dst_plane_width, out_w, rows,
                       bit_depth, stream ? (hipStream_t)stream : svtgpu_default_stream());
}

// svt_av1_superres_upscale_frame (EbRestProcess.c:405-458): the three planes, chroma widths rounded up
extern "C" int svtgpu_superres_upscale_frame(const SvtGpuFrame *src, SvtGpuFrame *dst, int32_t frame_width,
                                             int32_t upscaled_width, void *stream) {
    if (!src || !dst || src == dst || src->height != dst->height || src->bit_depth != dst->bit_depth ||
        frame_width <= 0 || frame_width > src->width || upscaled_width > dst->width || upscaled_width < frame_width ||
        2 * frame_width < upscaled_width)
        return SVTGPU_ERR_INVALID_ARG;
    hipStream_t st = pick_stream(dst->ctx, stream);
    const int   bs = src->bytes_per_sample;
    for (int p = 0; p < 3; p++) {
        const int sx = p > 0;
        if (frame_width == upscaled_width) { // unscaled: the columns both frames hold, as they are
            const int w = src->pw[p] < dst->pw[p] ? src->pw[p] : dst->pw[p];
            HIP_TRY(hipMemcpy2DAsync(dst->plane[p], (size_t)dst->stride[p] * bs, src->plane[p],
                                     (size_t)src->stride[p] * bs, (size_t)w * bs, src->ph[p],
                                     hipMemcpyDeviceToDevice, st));
            continue;
        }
        // the reference's right-edge replication starts at the downscaled frame's coded width (mi_cols * 4 >> sub_x)
        const int coded = ((frame_width + 7) & ~7) >> sx;
        if (int rc = upscale_dev(src->plane[p], bs * 8, src->stride[p], coded, (frame_width + sx) >> sx, dst->plane[p],
                                 dst->stride[p], dst->pw[p], (upscaled_width + sx) >> sx, src->ph[p], src->bit_depth,
                                 st))
            return rc;
    }
    return SVTGPU_OK;
}
