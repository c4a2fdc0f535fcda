// resize.hip — AV1's non-normative frame resizer on gfx950: svt_av1_resize_plane_c / svt_av1_highbd_resize_plane_c and
// their _horizontal variants (Source/Lib/Encoder/Codec/EbResize.c:148-737), the three planes of svt_aom_resize_frame
// (:887-973), and the RTCD shims of svt_av1_resize_plane / svt_av1_highbd_resize_plane.
//
// A plane is resized in two exact stages: every row from in_w to out_w, rounded and clipped to the sample range into
// intbuf[in_h][out_w], then every column of intbuf from in_h to out_h.  The clip in between is part of the result.  One
// 1-D resize (resize_multistep) is get_down2_steps halvings (svt_av1_down2_symeven on an even length, down2_symodd on an
// odd one) and then, if the length still differs, one svt_av1_interpolate_core.  Equal lengths are a copy.
//
// Every one of those 1-D operations is the same thing: output x is sum_k f[phase][k] * in[clamp((pos >> 14) - 3 + k)],
// k = 0..7, rounded by 7 bits and clipped, pos = pos0 + x * delta (14 fractional bits), phase = (pos >> 8) & 63.
//   interpolation   pos0 = offset + 128, delta = ((in << 14) + out / 2) / out, a 64-row table by the ratio
//   halving         pos0 = 0, delta = 2 << 14 (phase 0 always), the half filter mirrored about sample 2 * x:
//                   even length: taps 2x-3 .. 2x+4 = {f3 f2 f1 f0 f0 f1 f2 f3}; odd: 2x-3 .. 2x+3 = {f3 f2 f1 f0 f1 f2 f3}
// The reference's initial / middle / end parts and its short-input branches are all the index clamp to [0, in - 1].
// So there are two kernels, one along rows and one along columns, and a pass is one launch of one of them:
//
//   resize_h_kernel   a workgroup is 4 waves, one row each, kTileW = 512 outputs per wave.  A wave stages the source
//                     window of its outputs (at most 2 samples per output, plus the taps) once in LDS as 16-bit samples
//                     with 16-B loads on the aligned interior; the table is in LDS as rows of 8 packed int16.  A lane
//                     makes 8 adjacent outputs: per output five dwords from LDS, slid by 0 or 1 sample with
//                     v_alignbyte_b32, four v_dot2_i32_i16, and one wide store of the 8.
//   resize_v_kernel   lanes run along columns, 8 adjacent columns per lane (one 16-B / 8-B load per source row), a wave
//                     makes one output row, so the phase and the filter row are wave-uniform (scalar loads); the eight
//                     source rows of an output are read straight from memory (adjacent output rows of the workgroup
//                     share them through L2) and the 8 results stored at once.
// No scratch, no atomics.  Bounds: every source index is clamped to [0, in - 1] and every store is guarded by the
// output's width and height; the LDS window is sized for delta <= 2 << 14, which resize_plan guarantees.
//
// Workspace: intbuf and the two ping-pong buffers of multi-step halvings live in one growable device allocation per
// stream, kept for the life of the process.  It grows (stream synchronise + free + allocate) only when a call needs more
// than any call before it on that stream; otherwise a call allocates nothing.
#include <cstring>
#include <map>
#include <mutex>

#include "resize_tables.h"
#include "svtgpu_internal.h"

namespace {

constexpr int kOutPerLane = 8;
constexpr int kTileW      = 64 * kOutPerLane; // outputs of one wave (resize_h_kernel) / columns of one wave (resize_v_kernel)
constexpr int kRowsPerWg  = 4;
// samples of one wave's LDS window: the taps of kTileW outputs span at most 2 * (kTileW - 1) + 1 + 8 source samples
// (delta <= 2 << 14), the window starts up to 15 samples before them (16-B aligned loads of 8-bit samples), is filled in
// whole loads, and a lane reads ten samples from an even index: 1046 rounded up to 16, plus slack
constexpr int kWin    = 1072;
constexpr int kMaxDim = 65536; // positions have 14 fractional bits in an int32
constexpr int kTabUpscale = 4, kTabDown2Even = 5, kTabDown2Odd = 6;

typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

// one 1-D pass over a plane
struct Pass {
    const void *src;
    void       *dst;
    int32_t     src_stride, dst_stride; // samples
    int32_t     in_len, out_len;        // along the filtered direction
    int32_t     lines;                  // rows (horizontal pass) or columns (vertical pass)
    int32_t     pos0, delta, table, maxv;
    int32_t     src_aligned, dst_aligned; // every row starts at a multiple of a lane's access (16 B; 8 B for 8-bit columns)
};

__device__ __forceinline__ const uint4 *table_rows(int t, int *nrows) {
    if (t >= kTabDown2Even) {
        *nrows = 1;
        return (const uint4 *)kDown2Filter[t - kTabDown2Even];
    }
    *nrows = 64;
    return t == kTabUpscale ? (const uint4 *)kUpscaleFilter : (const uint4 *)kDownscaleFilter[t];
}

template <typename T>
__global__ __launch_bounds__(64 * kRowsPerWg) void resize_h_kernel(const Pass a) {
    constexpr int VEC = 16 / (int)sizeof(T); // samples of one 16-B load
    __shared__ __attribute__((aligned(16))) uint16_t win[kRowsPerWg][kWin];
    __shared__ uint4 filt[64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.y * kRowsPerWg + wave, X0 = blockIdx.x * kTileW;
    if (threadIdx.x < 64) {
        int          nr;
        const uint4 *t    = table_rows(a.table, &nr);
        filt[threadIdx.x] = t[(int)threadIdx.x < nr ? threadIdx.x : 0];
    }
    // the wave's source window [a0, a0 + n): first tap of its first output (rounded down to a 16-B load) .. last tap of
    // its last output
    const int last = a.out_len - 1;
    const int s_lo = ((a.pos0 + min(X0, last) * a.delta) >> 14) - 3;
    const int s_hi = ((a.pos0 + min(X0 + kTileW - 1, last) * a.delta) >> 14) + 4;
    const int a0   = s_lo & ~(VEC - 1); // floor to a multiple of VEC (two's complement, s_lo >= -4)
    const int n    = s_hi - a0 + 1;     // <= 2 * (kTileW - 1) + 8 + VEC
    if (y < a.lines) {
        const T  *row = (const T *)a.src + (size_t)y * a.src_stride;
        uint16_t *w   = win[wave];
        for (int c = lane * VEC; c < n; c += 64 * VEC) {
            const int b = a0 + c;
            if (a.src_aligned && b >= 0 && b + VEC <= a.in_len) {
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
            } else { // a plane edge or an unaligned row: one sample at a time, the index clamped
                for (int k = 0; k < VEC; k++) w[c + k] = (uint16_t)row[min(max(b + k, 0), a.in_len - 1)];
            }
        }
    }
    __syncthreads();

    const int X = X0 + lane * kOutPerLane;
    if (y >= a.lines || X >= a.out_len) return;
    const uint32_t *w32 = (const uint32_t *)win[wave];
    int             out[kOutPerLane];
#pragma unroll
    for (int j = 0; j < kOutPerLane; j++) {
        const int       pos = a.pos0 + min(X + j, last) * a.delta;
        const int       i   = (pos >> 14) - 3 - a0; // the first tap's window index, >= 0
        const uint32_t *q   = w32 + (i >> 1);       // ten samples from the even index at or below it
        const uint32_t  r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
        const uint32_t  sh = (uint32_t)(i & 1) * 2; // bytes to slide by
        const uint4     f  = filt[(pos >> 8) & 63];
        int             sum = dot2(__builtin_amdgcn_alignbyte(r1, r0, sh), f.x, 64);
        sum                 = dot2(__builtin_amdgcn_alignbyte(r2, r1, sh), f.y, sum);
        sum                 = dot2(__builtin_amdgcn_alignbyte(r3, r2, sh), f.z, sum);
        sum                 = dot2(__builtin_amdgcn_alignbyte(r4, r3, sh), f.w, sum);
        out[j]              = min(max(sum >> 7, 0), a.maxv);
    }
    T *d = (T *)a.dst + (size_t)y * a.dst_stride + X;
    if (a.dst_aligned && X + kOutPerLane <= a.out_len) {
        if (sizeof(T) == 2)
            *(uint4 *)d = make_uint4(out[0] | out[1] << 16, out[2] | out[3] << 16, out[4] | out[5] << 16,
                                     out[6] | out[7] << 16);
        else
            *(uint2 *)d = make_uint2(out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24,
                                     out[4] | out[5] << 8 | out[6] << 16 | out[7] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kOutPerLane; j++)
            if (X + j < a.out_len) d[j] = (T)out[j];
    }
}

template <typename T>
__global__ __launch_bounds__(64 * kRowsPerWg) void resize_v_kernel(const Pass a) {
    constexpr int VEC  = kOutPerLane; // columns of one lane
    const int     lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int     Y = blockIdx.y * kRowsPerWg + wave; // the output row: wave-uniform
    const int     X = (blockIdx.x * 64 + lane) * VEC;
    if (Y >= a.out_len || X >= a.lines) return;
    const int    pos = a.pos0 + Y * a.delta;
    const int    s   = (pos >> 14) - 3;
    int          nr;
    const uint4 *tab = table_rows(a.table, &nr);
    const uint4  f   = tab[nr > 1 ? (pos >> 8) & 63 : 0];
    const int    taps[8] = {(int16_t)(f.x & 0xffff), (int)f.x >> 16, (int16_t)(f.y & 0xffff), (int)f.y >> 16,
                            (int16_t)(f.z & 0xffff), (int)f.z >> 16, (int16_t)(f.w & 0xffff), (int)f.w >> 16};
    const bool   whole = X + VEC <= a.lines;
    int          acc[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) acc[c] = 64;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int r = min(max(s + k, 0), a.in_len - 1);
        const T  *p = (const T *)a.src + (size_t)r * a.src_stride + X;
        int       v[VEC];
        if (whole && a.src_aligned) {
            if (sizeof(T) == 2) {
                const uint4    q    = *(const uint4 *)p;
                const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int c = 0; c < 4; c++) v[2 * c] = (int)(u[c] & 0xffff), v[2 * c + 1] = (int)(u[c] >> 16);
            } else {
                const uint2    q    = *(const uint2 *)p;
                const uint32_t u[2] = {q.x, q.y};
#pragma unroll
                for (int c = 0; c < VEC; c++) v[c] = (int)((u[c >> 2] >> (8 * (c & 3))) & 0xff);
            }
        } else {
#pragma unroll
            for (int c = 0; c < VEC; c++) v[c] = X + c < a.lines ? (int)p[c] : 0;
        }
#pragma unroll
        for (int c = 0; c < VEC; c++) acc[c] += taps[k] * v[c];
    }
    int out[VEC];
#pragma unroll
    for (int c = 0; c < VEC; c++) out[c] = min(max(acc[c] >> 7, 0), a.maxv);
    T *d = (T *)a.dst + (size_t)Y * a.dst_stride + X;
    if (whole && a.dst_aligned) {
        if (sizeof(T) == 2)
            *(uint4 *)d = make_uint4(out[0] | out[1] << 16, out[2] | out[3] << 16, out[4] | out[5] << 16,
                                     out[6] | out[7] << 16);
        else
            *(uint2 *)d = make_uint2(out[0] | out[1] << 8 | out[2] << 16 | out[3] << 24,
                                     out[4] | out[5] << 8 | out[6] << 16 | out[7] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < VEC; c++)
            if (X + c < a.lines) d[c] = (T)out[c];
    }
}

// ---------------------------------------------------------------------------------------------
// the plan of one 1-D resize (resize_multistep, EbResize.c:353-387)
// ---------------------------------------------------------------------------------------------
struct Plan1D {
    int32_t steps, len, table, delta, offset; // len: the length that reaches the interpolation; table -1: none
};

bool plan_1d(int32_t in, int32_t out, Plan1D *p) {
    if (in <= 0 || out <= 0 || in > kMaxDim || out > kMaxDim || out > 2 * in) return false;
    *p = Plan1D{0, in, -1, 0, 0};
    if (in == out) return true;
    while (((p->len + 1) >> 1) >= out) { // get_down2_steps (:153-167)
        ++p->steps;
        p->len = (p->len + 1) >> 1;
        if (p->len == 1) break;
    }
    if (p->len == out) return true;
    const int32_t n = p->len, o16 = out * 16; // choose_interp_filter (:265-277), svt_av1_interpolate_core_c (:281-284)
    p->table  = o16 >= n * 16 ? kTabUpscale : o16 >= n * 13 ? 3 : o16 >= n * 11 ? 2 : o16 >= n * 9 ? 1 : 0;
    p->delta  = (int32_t)((((uint32_t)n << 14) + out / 2) / out);
    p->offset = n > out ? (((n - out) << 13) + out / 2) / out : -(((out - n) << 13) + out / 2) / out;
    return true;
}

int passes_of(const Plan1D &p) { return p.steps + (p.table >= 0); }

// ---------------------------------------------------------------------------------------------
// workspace: one growable allocation per stream
// ---------------------------------------------------------------------------------------------
struct Workspace {
    std::mutex m; // held while a call enqueues: two host threads on one stream take turns
    uint8_t   *d   = nullptr;
    size_t     cap = 0;
};
std::mutex                         g_ws_mutex;
std::map<hipStream_t, Workspace *> g_ws;

Workspace *workspace_of(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    Workspace                 *&w = g_ws[st];
    if (!w) w = new Workspace;
    return w;
}

int workspace_reserve(Workspace *w, hipStream_t st, size_t need) {
    if (need <= w->cap) return SVTGPU_OK;
    if (w->d) { // earlier calls on this stream may still read it
        HIP_TRY(hipStreamSynchronize(st));
        (void)hipFree(w->d);
        w->d = nullptr, w->cap = 0;
    }
    need = (need + (need >> 2) + 0xffff) & ~(size_t)0xffff;
    if (hipMalloc(&w->d, need) != hipSuccess) {
        w->d = nullptr;
        return SVTGPU_ERR_OOM;
    }
    w->cap = need;
    return SVTGPU_OK;
}

size_t row_stride(int w) { return ((size_t)w + 63) & ~(size_t)63; } // samples: rows of the workspace start 16-B aligned

int launch_pass(bool horizontal, int bits, Pass a, hipStream_t st) {
    const size_t bs   = bits / 8;
    const size_t unit = horizontal || bits == 16 ? 16 : 8;
    a.src_aligned     = !(((uintptr_t)a.src | ((size_t)a.src_stride * bs)) & (unit - 1));
    a.dst_aligned     = !(((uintptr_t)a.dst | ((size_t)a.dst_stride * bs)) & (kOutPerLane * bs - 1));
    const dim3 block(64 * kRowsPerWg);
    if (horizontal) {
        const dim3 grid((a.out_len + kTileW - 1) / kTileW, (a.lines + kRowsPerWg - 1) / kRowsPerWg);
        if (bits == 8)
            hipLaunchKernelGGL(resize_h_kernel<uint8_t>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(resize_h_kernel<uint16_t>, grid, block, 0, st, a);
    } else {
        const dim3 grid((a.lines + kTileW - 1) / kTileW, (a.out_len + kRowsPerWg - 1) / kRowsPerWg);
        if (bits == 8)
            hipLaunchKernelGGL(resize_v_kernel<uint8_t>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(resize_v_kernel<uint16_t>, grid, block, 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

// the passes of one direction: src (`len` samples along the direction) -> ... -> dst (`out` samples), through tmp[0] /
// tmp[1] when there are several
int run_direction(bool horizontal, int bits, const Plan1D &p, const void *src, int src_stride, int len, int out,
                  int lines, void *dst, int dst_stride, void *const tmp[2], int tmp_stride, int maxv, hipStream_t st) {
    const int   np  = passes_of(p);
    const void *cur = src;
    int         cs  = src_stride;
    for (int i = 0; i < np; i++) {
        const bool lastp = i == np - 1;
        Pass       a;
        a.src = cur, a.src_stride = cs, a.dst = lastp ? dst : tmp[i & 1], a.dst_stride = lastp ? dst_stride : tmp_stride;
        a.in_len = len, a.lines = lines, a.maxv = maxv;
        if (i < p.steps) // svt_av1_down2_symeven / down2_symodd
            a.out_len = (len + 1) >> 1, a.pos0 = 0, a.delta = 2 << 14, a.table = len & 1 ? kTabDown2Odd : kTabDown2Even;
        else // svt_av1_interpolate_core
            a.out_len = out, a.pos0 = p.offset + 128, a.delta = p.delta, a.table = p.table;
        if (a.delta > (2 << 14)) return SVTGPU_ERR_INVALID_ARG; // the LDS window's bound; plan_1d never gives more
        if (int rc = launch_pass(horizontal, bits, a, st)) return rc;
        cur = a.dst, cs = a.dst_stride, len = a.out_len;
    }
    return SVTGPU_OK;
}

bool sizes_ok(int bits, int src_stride, int in_w, int in_h, int dst_stride, int out_w, int out_h, int bit_depth,
              Plan1D *ph, Plan1D *pv) {
    if ((bits != 8 && bits != 16) || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0 || src_stride < in_w ||
        dst_stride < out_w || bit_depth < 8 || bit_depth > (bits == 8 ? 8 : 12))
        return false;
    return plan_1d(in_w, out_w, ph) && plan_1d(in_h, out_h, pv);
}

bool plane_args_ok(const void *src, int bits, int src_stride, int in_w, int in_h, const void *dst, int dst_stride,
                   int out_w, int out_h, int bit_depth, Plan1D *ph, Plan1D *pv) {
    if (!src || !dst || !sizes_ok(bits, src_stride, in_w, in_h, dst_stride, out_w, out_h, bit_depth, ph, pv))
        return false;
    const size_t    bs = bits / 8;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + ((size_t)(in_h - 1) * src_stride + in_w) * bs;
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + ((size_t)(out_h - 1) * dst_stride + out_w) * bs;
    return s1 <= d0 || d1 <= s0; // the buffers do not overlap
}

int resize_dev(const void *src, int bits, int src_stride, int in_w, int in_h, void *dst, int dst_stride, int out_w,
               int out_h, int bit_depth, hipStream_t st) {
    Plan1D ph, pv;
    if (!plane_args_ok(src, bits, src_stride, in_w, in_h, dst, dst_stride, out_w, out_h, bit_depth, &ph, &pv))
        return SVTGPU_ERR_INVALID_ARG;
    const size_t bs = bits / 8;
    const int    nh = passes_of(ph), nv = passes_of(pv), maxv = (1 << bit_depth) - 1;
    if (!nh && !nv) {
        HIP_TRY(hipMemcpy2DAsync(dst, dst_stride * bs, src, src_stride * bs, in_w * bs, in_h, hipMemcpyDeviceToDevice, st));
        return SVTGPU_OK;
    }
    // intbuf [in_h][out_w] between the stages; tmp[2] for the halvings before a direction's last pass
    const size_t int_stride = row_stride(out_w), int_bytes = nh && nv ? int_stride * in_h * bs : 0;
    const size_t tmp_h_stride = row_stride((in_w + 1) >> 1), tmp_v_stride = int_stride;
    const size_t tmp_h = nh > 1 ? tmp_h_stride * in_h * bs : 0, tmp_v = nv > 1 ? tmp_v_stride * ((in_h + 1) >> 1) * bs : 0;
    const size_t tmp_bytes = ((tmp_h > tmp_v ? tmp_h : tmp_v) + 255) & ~(size_t)255;
    const size_t int_off   = 2 * tmp_bytes;
    Workspace   *w = workspace_of(st);
    std::lock_guard<std::mutex> lk(w->m);
    if (int rc = workspace_reserve(w, st, int_off + int_bytes + 256)) return rc;
    void *const tmp[2] = {w->d, w->d + tmp_bytes};
    void       *mid    = nh && nv ? (void *)(w->d + int_off) : nullptr;
    if (nh)
        if (int rc = run_direction(true, bits, ph, src, src_stride, in_w, out_w, in_h, nv ? mid : dst,
                                   nv ? (int)int_stride : dst_stride, tmp, (int)tmp_h_stride, maxv, st))
            return rc;
    if (nv)
        if (int rc = run_direction(false, bits, pv, nh ? mid : src, nh ? (int)int_stride : src_stride, in_h, out_h, out_w,
                                   dst, dst_stride, tmp, (int)tmp_v_stride, maxv, st))
            return rc;
    return SVTGPU_OK;
}

// host planes through the calling thread's stage
template <typename T>
SVTGPU_ERROR_T shim_plane(const T *input, int height, int width, int in_stride, T *output, int height2, int width2,
                          int out_stride, int bd) {
    constexpr SVTGPU_ERROR_T kBadParameter = (SVTGPU_ERROR_T)0x80001005u; // EB_ErrorBadParameter
    if (!input || !output || width <= 0 || height <= 0 || width2 <= 0 || height2 <= 0 || in_stride < width ||
        out_stride < width2)
        return kBadParameter;
    const size_t ss = row_stride(width), ds = row_stride(width2), bs = sizeof(T);
    Carver       c;
    const size_t off_src = c(ss * height * bs), off_dst = c(ds * height2 * bs);
    Plan1D       ph, pv;
    if (!sizes_ok((int)bs * 8, (int)ss, width, height, (int)ds, width2, height2, bd, &ph, &pv)) return kBadParameter;
    hipStream_t st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    uint8_t *const d = sg.d + off_src;
    HIP_OR_DIE(hipMemcpy2DAsync(d, ss * bs, input, (size_t)in_stride * bs, (size_t)width * bs, height,
                                hipMemcpyHostToDevice, st));
    if (resize_dev(d, (int)bs * 8, (int)ss, width, height, sg.d + off_dst, (int)ds, width2, height2, bd, st))
        svtgpu_fatal("svtgpu resize shim: the device resize failed");
    HIP_OR_DIE(hipMemcpy2DAsync(output, (size_t)out_stride * bs, sg.d + off_dst, ds * bs, (size_t)width2 * bs, height2,
                                hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    return (SVTGPU_ERROR_T)0;
}

} // namespace

// ---------------------------------------------------------------------------------------------
// host-only entry points
// ---------------------------------------------------------------------------------------------
extern "C" int svtgpu_resize_plan(int32_t in_length, int32_t out_length, int32_t *steps, int32_t *filter_index,
                                  int32_t *delta, int32_t *offset) {
    Plan1D p;
    if (!steps || !filter_index || !delta || !offset || !plan_1d(in_length, out_length, &p)) return SVTGPU_ERR_INVALID_ARG;
    *steps = p.steps, *filter_index = p.table, *delta = p.delta, *offset = p.offset;
    return SVTGPU_OK;
}

extern "C" int svtgpu_resize_filter(int32_t filter_index, int16_t out[64][8]) {
    if (!out || filter_index < 0 || filter_index > kTabUpscale) return SVTGPU_ERR_INVALID_ARG;
    memcpy(out, filter_index == kTabUpscale ? kUpscaleFilter : kDownscaleFilter[filter_index], sizeof(int16_t) * 64 * 8);
    return SVTGPU_OK;
}

extern "C" int svtgpu_resize_half_filters(int16_t symeven[4], int16_t symodd[4]) {
    if (!symeven || !symodd) return SVTGPU_ERR_INVALID_ARG;
    memcpy(symeven, kDown2HalfFilter[0], sizeof(int16_t) * 4);
    memcpy(symodd, kDown2HalfFilter[1], sizeof(int16_t) * 4);
    return SVTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// device entry points
// ---------------------------------------------------------------------------------------------
extern "C" int svtgpu_resize_plane(const void *src, int32_t bits, int32_t src_stride, int32_t in_w, int32_t in_h,
                                   void *dst, int32_t dst_stride, int32_t out_w, int32_t out_h, int32_t bit_depth,
                                   void *stream) {
    Plan1D ph, pv; // refused before the default stream (and with it a device) is asked for
    if (!plane_args_ok(src, bits, src_stride, in_w, in_h, dst, dst_stride, out_w, out_h, bit_depth, &ph, &pv))
        return SVTGPU_ERR_INVALID_ARG;
    return resize_dev(src, bits, src_stride, in_w, in_h, dst, dst_stride, out_w, out_h, bit_depth,
                      stream ? (hipStream_t)stream : svtgpu_default_stream());
}

// svt_aom_resize_frame (EbResize.c:887-973): the three planes, chroma sizes (dim + 1) >> 1 on both sides
extern "C" int svtgpu_resize_frame(const SvtGpuFrame *src, SvtGpuFrame *dst, int32_t src_w, int32_t src_h, int32_t dst_w,
                                   int32_t dst_h, void *stream) {
    if (!src || !dst || src == dst || src->bit_depth != dst->bit_depth || src_w <= 0 || src_h <= 0 || dst_w <= 0 ||
        dst_h <= 0 || src_w > src->width || src_h > src->height || dst_w > dst->width || dst_h > dst->height)
        return SVTGPU_ERR_INVALID_ARG;
    const int bits = src->bytes_per_sample * 8;
    for (int p = 0; p < 3; p++) { // every plane's arguments before the first launch
        const int s = p > 0;
        Plan1D    ph, pv;
        if (!plane_args_ok(src->plane[p], bits, src->stride[p], (src_w + s) >> s, (src_h + s) >> s, dst->plane[p],
                           dst->stride[p], (dst_w + s) >> s, (dst_h + s) >> s, src->bit_depth, &ph, &pv))
            return SVTGPU_ERR_INVALID_ARG;
    }
    hipStream_t st = pick_stream(dst->ctx, stream);
    for (int p = 0; p < 3; p++) {
        const int s = p > 0;
        if (int rc = resize_dev(src->plane[p], bits, src->stride[p], (src_w + s) >> s, (src_h + s) >> s, dst->plane[p],
                                dst->stride[p], (dst_w + s) >> s, (dst_h + s) >> s, src->bit_depth, st))
            return rc;
    }
    return SVTGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// RTCD shims (aom_dsp_rtcd.h:898-901): host pointers, synchronous
// ---------------------------------------------------------------------------------------------
extern "C" SVTGPU_ERROR_T svtgpu_av1_resize_plane(const uint8_t *const input, int height, int width, int in_stride,
                                                  uint8_t *output, int height2, int width2, int out_stride) {
    return shim_plane<uint8_t>(input, height, width, in_stride, output, height2, width2, out_stride, 8);
}

extern "C" SVTGPU_ERROR_T svtgpu_av1_highbd_resize_plane(const uint16_t *const input, int height, int width,
                                                         int in_stride, uint16_t *output, int height2, int width2,
                                                         int out_stride, int bd) {
    return shim_plane<uint16_t>(input, height, width, in_stride, output, height2, width2, out_stride, bd);
}
