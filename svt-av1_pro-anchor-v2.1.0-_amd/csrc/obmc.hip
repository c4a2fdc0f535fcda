// obmc.hip — the overlapped-block motion compensation (OBMC) distortion family on gfx950.
//
// Reference (Source/Lib/Encoder/): C_DEFAULT/sad_av1.c:18-62 (obmc_sad), C_DEFAULT/variance.c:347-451 (obmc_variance,
// OBMC_VAR, OBMC_SUBPIX_VAR), Codec/av1me.c:709-776 (get_obmc_mvpred_var, obmc_refining_search_sad,
// svt_av1_obmc_full_pixel_search) with the costs of av1me.c:237-261.  8-bit only, as in the reference.
//
//   diff(x) = wsrc[x] - pre[x] * mask[x]          (wsrc, mask: compact W x H int32, scaled by 4096)
//   SAD     = sum (|diff| + 2048) >> 12
//   var     = sse - (uint32)((int64)sum * sum / (W * H)) over d = sign(diff) * ((|diff| + 2048) >> 12)
//
// Per-block shims (svtgpu_aom_obmc_*): one staging copy, one launch of obmc_block_kernel (one workgroup; the sub-pel
// form filters the (H + 1) x (W + 1) window through LDS first), one 12-byte read-back.
//
// Batch (svtgpu_obmc_search): one 256-lane workgroup per item walks the whole refinement on the device.  The reference
// window the walk can reach -- the clamped start +- search_range, plus one row / four columns of padding so every
// step reads whole dwords -- is staged once in LDS (at most 162 rows x 172 bytes).  Each lane owns quads of four
// horizontally adjacent samples (W is a multiple of 4) and keeps their wsrc / mask values in registers for the whole
// walk: 1, 4 or 16 quads per lane, three instantiations of the kernel, each workgroup of a launch leaving at once when
// its item belongs to another one.  A step reads, per quad, three dwords of each of the three window rows around the
// current position and forms the 4 or 8 neighbours' samples with v_alignbyte; the neighbours' SADs reduce in the waves
// with DPP adds and across the four waves through LDS, and every lane then applies the reference's sequential take-over
// rule to the same totals, so the new position needs no second exchange: one barrier per step.
#include <algorithm>
#include <cstring>
#include <vector>

#include "svtgpu_internal.h"

namespace {

constexpr int kMaxRange  = SVTGPU_OBMC_MAX_RANGE;
constexpr int kWinStride = 128 + 2 * kMaxRange + 12; // bytes per LDS window row
constexpr int kWinRows   = 128 + 2 * kMaxRange + 2;

__device__ __forceinline__ uint32_t obmc_abs_round(int wsrc, int pre, int mask) {
    return (uint32_t)((abs(wsrc - pre * mask) + 2048) >> 12);
}
__device__ __forceinline__ int obmc_diff(int wsrc, int pre, int mask) { // ROUND_POWER_OF_TWO_SIGNED(.., 12)
    const int v = wsrc - pre * mask, r = (abs(v) + 2048) >> 12;
    return v < 0 ? -r : r;
}

// sum over the workgroup of up to 9 per-lane values: slot[wave][j] receives the wave totals (mod 2^32)
__device__ __forceinline__ void wave_totals(uint32_t need, const uint32_t (&acc)[9], uint32_t (*slot)[9]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 9; j++)
        if ((need >> j) & 1) {
            const uint32_t v = wave_sum_u32_lane63(acc[j]);
            if (lane == 63) slot[wave][j] = v;
        }
}

// ---------------------------------------------------------------------------------------------
// per-block shims
// ---------------------------------------------------------------------------------------------
// out = {SAD, sum, sse} of one block.  subpel: pre is the (h + 1) x (w + 1) window (stride w + 1) and the block is
// its 2-tap bilinear interpolation (first pass over h + 1 rows to 16 bits, second pass to 8 bits, variance.c:375-390)
__global__ __launch_bounds__(256) void obmc_block_kernel(const uint8_t *pre, const int32_t *wsrc, const int32_t *mask,
                                                         int w, int h, int subpel, int xoff, int yoff, uint32_t *out) {
    __shared__ uint16_t f1[129 * 128];
    __shared__ uint32_t red[4][9];
    const int fx0 = 128 - 16 * xoff, fx1 = 16 * xoff, fy0 = 128 - 16 * yoff, fy1 = 16 * yoff;
    if (subpel) {
        const int as = w + 1;
        for (int i = threadIdx.x; i < (h + 1) * w; i += 256) {
            const int r = i / w, c = i - r * w;
            f1[i] = (uint16_t)(((int)pre[r * as + c] * fx0 + (int)pre[r * as + c + 1] * fx1 + 64) >> 7);
        }
        __syncthreads();
    }
    uint32_t acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < w * h; i += 256) {
        const int p = subpel ? (int)(uint8_t)(((int)f1[i] * fy0 + (int)f1[i + w] * fy1 + 64) >> 7) : (int)pre[i];
        const int d = obmc_diff(wsrc[i], p, mask[i]);
        acc[0] += obmc_abs_round(wsrc[i], p, mask[i]);
        acc[1] += (uint32_t)d;
        acc[2] += (uint32_t)(d * d);
    }
    wave_totals(7u, acc, red);
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

struct Totals {
    uint32_t sad;
    int32_t  sum;
    uint32_t sse;
};

// stages {wsrc, mask, result, pre rows} on the calling thread's stage with one copy, runs the kernel, reads the 12-byte
// result back
Totals obmc_block(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, int w, int h, int subpel,
                  int xoff, int yoff) {
    const size_t n = (size_t)w * h, pw = subpel ? w + 1 : w, ph = subpel ? h + 1 : h;
    Carver       c;
    const size_t off_wsrc = c(n * 4), off_mask = c(n * 4), off_out = c(16), off_pre = c(pw * ph);
    hipStream_t  st = svtgpu_shim_stream();
    const SvtGpuStageLease sg = svtgpu_stage_reserve(c.off, st);
    memcpy(sg.h + off_wsrc, wsrc, n * 4);
    memcpy(sg.h + off_mask, mask, n * 4);
    memset(sg.h + off_out, 0, 16);
    for (size_t r = 0; r < ph; r++) memcpy(sg.h + off_pre + r * pw, pre + (ptrdiff_t)r * pre_stride, pw);
    HIP_OR_DIE(hipMemcpyAsync(sg.d + off_wsrc, sg.h + off_wsrc, c.off - off_wsrc, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(obmc_block_kernel, dim3(1), dim3(256), 0, st, sg.d + off_pre, sg.dev<const int32_t>(off_wsrc),
                       sg.dev<const int32_t>(off_mask), w, h, subpel, xoff & 7, yoff & 7, sg.dev<uint32_t>(off_out));
    HIP_OR_DIE(hipGetLastError());
    uint32_t r[3];
    HIP_OR_DIE(hipMemcpyAsync(r, sg.d + off_out, sizeof r, hipMemcpyDeviceToHost, st));
    HIP_OR_DIE(hipStreamSynchronize(st));
    return {r[0], (int32_t)r[1], r[2]};
}

unsigned int obmc_var(const Totals &t, int n, unsigned int *sse) { // OBMC_VAR (variance.c:367-373)
    *sse = t.sse;
    return *sse - (unsigned int)(((int64_t)t.sum * t.sum) / n);
}

// ---------------------------------------------------------------------------------------------
// batched full-pel search
// ---------------------------------------------------------------------------------------------
struct ObmcArgs {
    const SvtGpuObmcItem *items;
    const int32_t        *wm, *cost;
    SvtGpuObmcResult     *out;
    const uint8_t        *ref[8];
    int32_t               ref_stride[8];
    int32_t               width, height, item_begin;
};

// quads of four samples per lane: the kernel instantiation an item of n samples runs in
__host__ __device__ inline int quads_per_lane(int n) { return n <= 1024 ? 1 : n <= 4096 ? 4 : 16; }

__device__ __forceinline__ uint32_t quad_sad(uint32_t pix, const int4 &w, const int4 &m) {
    return obmc_abs_round(w.x, (int)(pix & 0xFF), m.x) + obmc_abs_round(w.y, (int)((pix >> 8) & 0xFF), m.y) +
           obmc_abs_round(w.z, (int)((pix >> 16) & 0xFF), m.z) + obmc_abs_round(w.w, (int)(pix >> 24), m.w);
}

// mvsad_err_cost (av1me.c:254-261) of the full-pel MV (row, col); fr / fc = the centre >> 3; r0 / c0 = the first
// row / column of the item's cost tables (the clamped start - search_range)
__device__ __forceinline__ uint32_t obmc_mv_cost(const SvtGpuObmcItem &it, const int32_t *tab, int row, int col, int fr,
                                                 int fc, int r0, int c0) {
    const int dr = row - fr, dc = col - fc;
    if (it.cost_mode == 0) // mvsad_err_cost_light (av1me.c:237-243)
        return 1296u + 50u * ((uint32_t)abs(dc) * 8u + (uint32_t)abs(dr) * 8u);
    const int      nt   = 2 * it.search_range + 1;
    const int      j    = dr == 0 ? (dc == 0 ? 0 : 1) : (dc == 0 ? 2 : 3); // svt_av1_get_mv_joint
    const uint32_t bits = (uint32_t)(tab[j] + tab[4 + row - r0] + tab[4 + nt + col - c0]);
    return (bits * (uint32_t)it.sad_per_bit + 256u) >> 9; // ROUND_POWER_OF_TWO(.., AV1_PROB_COST_SHIFT)
}

// the neighbours in the reference's order (av1me.c:724) and the slot of each (row, col) offset of the 3 x 3
// neighbourhood; slot 8 is the position itself
#define OBMC_NB_ROW {-1, 0, 0, 1, -1, 1, 1, -1}
#define OBMC_NB_COL {0, -1, 1, 0, 1, 1, -1, -1}
#define OBMC_SLOT {{7, 0, 4}, {1, 8, 2}, {6, 3, 5}}

template <int Q>
__global__ __launch_bounds__(256) void obmc_search_kernel(const ObmcArgs A) {
    __shared__ __align__(16) uint8_t win[kWinRows * kWinStride];
    __shared__ uint32_t             part[3][4][9];
    constexpr int nb_row[8] = OBMC_NB_ROW, nb_col[8] = OBMC_NB_COL, slot[3][3] = OBMC_SLOT;
    const SvtGpuObmcItem it = A.items[A.item_begin + blockIdx.x];
    const int W = it.w, H = it.h, n = W * H;
    if (quads_per_lane(n) != Q) return; // another instantiation's item (uniform over the workgroup)
    const int tid = threadIdx.x, R = it.search_range;
    const int nq = n >> 2, lgq = 31 - __clz(W >> 2), qmask = (W >> 2) - 1, nk = (nq + 255) >> 8;
    // clamp_mv (av1me.c:768)
    const int sr = min(max(it.mvp_row, it.row_min), it.row_max), sc = min(max(it.mvp_col, it.col_min), it.col_max);
    const int fr = it.ref_mv_row >> 3, fc = it.ref_mv_col >> 3;
    const int32_t *tab = A.cost + it.cost_offset;

    // the lane's wsrc / mask quads; a lane past the block holds zeros, which add nothing to any sum
    int4 ws[Q], mk[Q];
#pragma unroll
    for (int k = 0; k < Q; k++) {
        const int q = k * 256 + tid;
        ws[k] = mk[k] = make_int4(0, 0, 0, 0);
        if (q < nq) {
            ws[k] = *(const int4 *)(A.wm + it.wm_offset + 4 * q);
            mk[k] = *(const int4 *)(A.wm + it.wm_offset + n + 4 * q);
        }
    }
    // window sample (0, 0) = reference sample (y + sr - R - 1, x + sc - R - 4); outside the frame: the nearest edge
    {
        const uint8_t *ref = A.ref[it.ref];
        const int      rs = A.ref_stride[it.ref], rows = H + 2 * R + 2, colsq = (W + 2 * R + 12 + 3) >> 2;
        const int      fy0 = it.y + sr - R - 1, fx0 = it.x + sc - R - 4;
        for (int i = tid; i < rows * colsq; i += 256) {
            const int rr = i / colsq, cq = i - rr * colsq;
            const int y  = min(max(fy0 + rr, 0), A.height - 1);
            uint32_t  v  = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int x = min(max(fx0 + 4 * cq + c, 0), A.width - 1);
                v |= (uint32_t)ref[(size_t)y * rs + x] << (8 * c);
            }
            *(uint32_t *)(win + rr * kWinStride + 4 * cq) = v;
        }
    }
    __syncthreads();

    // SADs of the slots in `need` around the position (cr, cc) relative to the start
    auto eval = [&](uint32_t need, int cr, int cc, uint32_t(&acc)[9]) {
        const int cb = R + cc + 3, m = cb & 3; // window column of sample 0 at column offset -1, and its misalignment
#pragma unroll
        for (int j = 0; j < 9; j++) acc[j] = 0;
#pragma unroll
        for (int k = 0; k < Q; k++) {
            if (k >= nk) continue; // uniform: the block has fewer quads
            const int      q = min(k * 256 + tid, nq - 1), py = q >> lgq, px = (q & qmask) << 2;
            const uint8_t *p0 = win + (py + R + cr) * kWinStride + ((px + cb) & ~3);
#pragma unroll
            for (int dr = 0; dr < 3; dr++) {
                const uint32_t *p  = (const uint32_t *)(p0 + dr * kWinStride);
                const uint32_t  d0 = p[0], d1 = p[1], d2 = p[2];
#pragma unroll
                for (int dc = 0; dc < 3; dc++) {
                    const int j = slot[dr][dc];
                    if ((need >> j) & 1) {
                        const int      t   = m + dc;
                        const uint32_t pix = t < 4 ? __builtin_amdgcn_alignbyte(d1, d0, t)
                                                   : __builtin_amdgcn_alignbyte(d2, d1, t - 4);
                        acc[j] += quad_sad(pix, ws[k], mk[k]);
                    }
                }
            }
        }
    };
    auto total = [&](int buf, int j) { return part[buf][0][j] + part[buf][1][j] + part[buf][2][j] + part[buf][3][j]; };

    uint32_t acc[9];
    eval(1u << 8, 0, 0, acc);
    wave_totals(1u << 8, acc, part[0]);
    __syncthreads();
    uint32_t best = total(0, 8) + obmc_mv_cost(it, tab, sr, sc, fr, fc, sr - R, sc - R);
    int      cr = 0, cc = 0, steps = 0;
    const uint32_t need  = it.search_diag ? 0xFFu : 0x0Fu;
    for (int i = 0; i < R; i++) {
        const int buf = (i + 1) & 1; // the other buffer may still be read by a slower wave
        eval(need, cr, cc, acc);
        wave_totals(need, acc, part[buf]);
        __syncthreads();
        // every lane applies the sequential rule to the same totals (av1me.c:735-748)
        int tr = 0, tc = 0, site = -1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (!((need >> j) & 1)) continue;
            const int row = sr + cr + nb_row[j], col = sc + cc + nb_col[j];
            if (col < it.col_min || col > it.col_max || row < it.row_min || row > it.row_max) continue;
            uint32_t sad = total(buf, j);
            if (sad < best) {
                sad += obmc_mv_cost(it, tab, row, col, fr, fc, sr - R, sc - R);
                if (sad < best) best = sad, site = j, tr = nb_row[j], tc = nb_col[j];
            }
        }
        if (site < 0) break;
        cr += tr, cc += tc, steps++;
    }
    // the OBMC variance at the final position (get_obmc_mvpred_var, av1me.c:709-720, without its MV cost)
    uint32_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
        const int cb = R + cc + 4, m = cb & 3;
#pragma unroll
        for (int k = 0; k < Q; k++) {
            if (k >= nk) continue;
            const int       q = min(k * 256 + tid, nq - 1), py = q >> lgq, px = (q & qmask) << 2;
            const uint32_t *p = (const uint32_t *)(win + (py + R + cr + 1) * kWinStride + ((px + cb) & ~3));
            const uint32_t  pix = __builtin_amdgcn_alignbyte(p[1], p[0], m);
            const int d0 = obmc_diff(ws[k].x, (int)(pix & 0xFF), mk[k].x);
            const int d1 = obmc_diff(ws[k].y, (int)((pix >> 8) & 0xFF), mk[k].y);
            const int d2 = obmc_diff(ws[k].z, (int)((pix >> 16) & 0xFF), mk[k].z);
            const int d3 = obmc_diff(ws[k].w, (int)(pix >> 24), mk[k].w);
            v[0] += (uint32_t)(d0 + d1 + d2 + d3);
            v[1] += (uint32_t)(d0 * d0) + (uint32_t)(d1 * d1) + (uint32_t)(d2 * d2) + (uint32_t)(d3 * d3);
        }
    }
    wave_totals(3u, v, part[2]);
    __syncthreads();
    if (tid == 0) {
        const int32_t    sum = (int32_t)total(2, 0);
        const uint32_t   sse = total(2, 1);
        SvtGpuObmcResult r;
        r.mv_col   = sc + cc;
        r.mv_row   = sr + cr;
        r.best_sad = best;
        r.variance = sse - (uint32_t)(((int64_t)sum * sum) / n);
        r.sse      = sse;
        r.steps    = steps;
        A.out[A.item_begin + blockIdx.x] = r;
    }
}

bool obmc_size_ok(int w, int h) {
    static const int sizes[22][2] = {{4, 4},   {4, 8},   {8, 4},    {8, 8},    {8, 16},    {16, 8}, {16, 16}, {16, 32},
                                     {32, 16}, {32, 32}, {32, 64},  {64, 32},  {64, 64},   {64, 128}, {128, 64},
                                     {128, 128}, {4, 16}, {16, 4},  {8, 32},   {32, 8},    {16, 64}, {64, 16}};
    for (const auto &s : sizes)
        if (s[0] == w && s[1] == h) return true;
    return false;
}

} // namespace

#define OBMC_SIZE_SHIMS(W, H)                                                                                      \
    extern "C" unsigned int svtgpu_aom_obmc_sad##W##x##H(const uint8_t *pre, int pre_stride, const int32_t *wsrc,  \
                                                         const int32_t *mask) {                                    \
        return obmc_block(pre, pre_stride, wsrc, mask, W, H, 0, 0, 0).sad;                                         \
    }                                                                                                              \
    extern "C" unsigned int svtgpu_aom_obmc_variance##W##x##H(const uint8_t *pre, int pre_stride,                  \
                                                              const int32_t *wsrc, const int32_t *mask,            \
                                                              unsigned int *sse) {                                 \
        return obmc_var(obmc_block(pre, pre_stride, wsrc, mask, W, H, 0, 0, 0), W * H, sse);                       \
    }                                                                                                              \
    extern "C" unsigned int svtgpu_aom_obmc_sub_pixel_variance##W##x##H(const uint8_t *pre, int pre_stride,        \
                                                                        int xoffset, int yoffset,                  \
                                                                        const int32_t *wsrc, const int32_t *mask,  \
                                                                        unsigned int *sse) {                       \
        return obmc_var(obmc_block(pre, pre_stride, wsrc, mask, W, H, 1, xoffset, yoffset), W * H, sse);           \
    }
OBMC_SIZE_SHIMS(4, 4)
OBMC_SIZE_SHIMS(4, 8)
OBMC_SIZE_SHIMS(8, 4)
OBMC_SIZE_SHIMS(8, 8)
OBMC_SIZE_SHIMS(8, 16)
OBMC_SIZE_SHIMS(16, 8)
OBMC_SIZE_SHIMS(16, 16)
OBMC_SIZE_SHIMS(16, 32)
OBMC_SIZE_SHIMS(32, 16)
OBMC_SIZE_SHIMS(32, 32)
OBMC_SIZE_SHIMS(32, 64)
OBMC_SIZE_SHIMS(64, 32)
OBMC_SIZE_SHIMS(64, 64)
OBMC_SIZE_SHIMS(64, 128)
OBMC_SIZE_SHIMS(128, 64)
OBMC_SIZE_SHIMS(128, 128)
OBMC_SIZE_SHIMS(4, 16)
OBMC_SIZE_SHIMS(16, 4)
OBMC_SIZE_SHIMS(8, 32)
OBMC_SIZE_SHIMS(32, 8)
OBMC_SIZE_SHIMS(16, 64)
OBMC_SIZE_SHIMS(64, 16)

// ---------------------------------------------------------------------------------------------
// batch object
// ---------------------------------------------------------------------------------------------
struct SvtGpuObmcBatch {
    SvtGpuContext    *ctx;
    int32_t           width, height, nref, max_items, nitems;
    int32_t           nclass[3]; // items of each kernel instantiation (1, 4, 16 quads per lane)
    SvtGpuObmcItem   *d_items;
    SvtGpuObmcResult *d_out;
    int32_t          *d_wm, *d_cost;
    size_t            wm_cap, cost_cap; // int32 entries
};

extern "C" int svtgpu_obmc_batch_create(SvtGpuContext *ctx, int32_t width, int32_t height, int32_t nref,
                                        int32_t max_items, SvtGpuObmcBatch **out) {
    if (!ctx || !out || width <= 0 || height <= 0 || nref < 1 || nref > 8 || max_items < 1)
        return SVTGPU_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    SvtGpuObmcBatch *b = new SvtGpuObmcBatch();
    b->ctx = ctx, b->width = width, b->height = height, b->nref = nref, b->max_items = max_items;
    hipError_t e = hipMalloc(&b->d_items, (size_t)max_items * sizeof(SvtGpuObmcItem));
    if (e == hipSuccess) e = hipMalloc(&b->d_out, (size_t)max_items * sizeof(SvtGpuObmcResult));
    if (e != hipSuccess) {
        svtgpu_obmc_batch_destroy(b);
        svtgpu_set_last_hip_error(e, "obmc batch alloc", __FILE__, __LINE__);
        return e == hipErrorOutOfMemory ? SVTGPU_ERR_OOM : SVTGPU_ERR_HIP;
    }
    *out = b;
    return SVTGPU_OK;
}

extern "C" void svtgpu_obmc_batch_destroy(SvtGpuObmcBatch *b) {
    if (!b) return;
    (void)hipFree(b->d_items);
    (void)hipFree(b->d_out);
    (void)hipFree(b->d_wm);
    (void)hipFree(b->d_cost);
    delete b;
}

// svtgpu_obmc_set_items, and svtgpu_obmc_set_items_device_wm when wm_dev is set: then the pool is sized and its address handed
// out, but nothing is uploaded into it (svtgpu_obmc_weighted_src_batch fills it on the device)
static int set_items(SvtGpuObmcBatch *b, const SvtGpuObmcItem *items, int32_t nitems, const int32_t *wm_pool, int32_t wm_count,
                     const int32_t *cost_pool, int32_t cost_count, int32_t **wm_dev, void *stream) {
    if (!b || nitems < 0 || nitems > b->max_items || (nitems && (!items || (!wm_pool && !wm_dev))) || wm_count < 0 ||
        cost_count < 0 || (cost_count && !cost_pool))
        return SVTGPU_ERR_INVALID_ARG;
    b->nitems = 0; // a rejected list leaves nothing to search
    int32_t nclass[3] = {0, 0, 0};
    for (int i = 0; i < nitems; i++) {
        const SvtGpuObmcItem &t = items[i];
        constexpr int         lim = 1 << 14; // MV_UPP: keeps every coordinate sum far inside int32
        if (!obmc_size_ok(t.w, t.h) || t.ref < 0 || t.ref >= b->nref || t.search_range < 0 ||
            t.search_range > kMaxRange || t.x < 0 || t.y < 0 || t.x >= b->width || t.y >= b->height ||
            t.col_min > t.col_max || t.row_min > t.row_max || t.col_min < -lim || t.col_max > lim ||
            t.row_min < -lim || t.row_max > lim || (t.cost_mode != 0 && t.cost_mode != 1) || t.wm_offset < 0 ||
            (t.wm_offset & 3) || (int64_t)t.wm_offset + 2 * t.w * t.h > wm_count)
            return SVTGPU_ERR_INVALID_ARG;
        if (t.cost_mode == 1 &&
            (t.cost_offset < 0 || (int64_t)t.cost_offset + 4 + 2 * (2 * t.search_range + 1) > cost_count))
            return SVTGPU_ERR_INVALID_ARG;
        const int q = quads_per_lane(t.w * t.h);
        nclass[q == 1 ? 0 : q == 4 ? 1 : 2]++;
    }
    hipStream_t st = pick_stream(b->ctx, stream);
    HIP_TRY(hipSetDevice(b->ctx->device));
    auto grow = [&](int32_t *&d, size_t &cap, size_t need) -> hipError_t {
        if (need <= cap) return hipSuccess;
        hipError_t e = hipStreamSynchronize(st); // an earlier search may still read the old pool
        if (e != hipSuccess) return e;
        (void)hipFree(d);
        d = nullptr, cap = 0;
        e = hipMalloc(&d, need * sizeof(int32_t));
        if (e == hipSuccess) cap = need;
        return e;
    };
    HIP_TRY(grow(b->d_wm, b->wm_cap, (size_t)wm_count));
    HIP_TRY(grow(b->d_cost, b->cost_cap, (size_t)cost_count));
    if (nitems) HIP_TRY(hipMemcpyAsync(b->d_items, items, (size_t)nitems * sizeof *items, hipMemcpyHostToDevice, st));
    if (wm_count && !wm_dev)
        HIP_TRY(hipMemcpyAsync(b->d_wm, wm_pool, (size_t)wm_count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (cost_count)
        HIP_TRY(hipMemcpyAsync(b->d_cost, cost_pool, (size_t)cost_count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    svtgpu_count_xfer(0, (size_t)nitems * sizeof *items + ((size_t)(wm_dev ? 0 : wm_count) + cost_count) * sizeof(int32_t));
    HIP_TRY(hipStreamSynchronize(st));
    b->nitems = nitems;
    std::memcpy(b->nclass, nclass, sizeof nclass);
    if (wm_dev) *wm_dev = b->d_wm;
    return SVTGPU_OK;
}

extern "C" int svtgpu_obmc_set_items(SvtGpuObmcBatch *b, const SvtGpuObmcItem *items, int32_t nitems,
                                     const int32_t *wm_pool, int32_t wm_count, const int32_t *cost_pool,
                                     int32_t cost_count, void *stream) {
    return set_items(b, items, nitems, wm_pool, wm_count, cost_pool, cost_count, nullptr, stream);
}

extern "C" int svtgpu_obmc_set_items_device_wm(SvtGpuObmcBatch *b, const SvtGpuObmcItem *items, int32_t nitems, int32_t wm_count,
                                               const int32_t *cost_pool, int32_t cost_count, int32_t **wm_dev, void *stream) {
    if (!wm_dev) return SVTGPU_ERR_INVALID_ARG;
    return set_items(b, items, nitems, nullptr, wm_count, cost_pool, cost_count, wm_dev, stream);
}

extern "C" int svtgpu_obmc_search(SvtGpuObmcBatch *b, const SvtGpuFrame *const *refs, int32_t item_begin,
                                  int32_t item_end, void *stream) {
    if (!b || !refs || item_begin < 0 || item_end > b->nitems || item_begin > item_end) return SVTGPU_ERR_INVALID_ARG;
    ObmcArgs a;
    std::memset(&a, 0, sizeof a);
    for (int r = 0; r < b->nref; r++) {
        const SvtGpuFrame *f = refs[r];
        if (!f || f->width != b->width || f->height != b->height) return SVTGPU_ERR_INVALID_ARG;
        if (f->bit_depth != 8) return SVTGPU_ERR_UNSUPPORTED; // the reference has no high-bit-depth OBMC kernels
        a.ref[r] = (const uint8_t *)f->plane[0], a.ref_stride[r] = f->stride[0];
    }
    a.items = b->d_items, a.wm = b->d_wm, a.cost = b->d_cost, a.out = b->d_out;
    a.width = b->width, a.height = b->height, a.item_begin = item_begin;
    if (item_end == item_begin) return SVTGPU_OK;
    hipStream_t st = pick_stream(b->ctx, stream);
    const dim3  grid(item_end - item_begin), block(256);
    // one launch per instantiation the list needs; a workgroup whose item belongs to another one leaves at once
    if (b->nclass[0]) hipLaunchKernelGGL(obmc_search_kernel<1>, grid, block, 0, st, a);
    if (b->nclass[1]) hipLaunchKernelGGL(obmc_search_kernel<4>, grid, block, 0, st, a);
    if (b->nclass[2]) hipLaunchKernelGGL(obmc_search_kernel<16>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return SVTGPU_OK;
}

extern "C" int svtgpu_obmc_read(SvtGpuObmcBatch *b, SvtGpuObmcResult *out, int32_t item_begin, int32_t item_end,
                                void *stream) {
    if (!b || !out || item_begin < 0 || item_end > b->nitems || item_begin > item_end) return SVTGPU_ERR_INVALID_ARG;
    hipStream_t  st = pick_stream(b->ctx, stream);
    const size_t n  = (size_t)(item_end - item_begin) * sizeof(SvtGpuObmcResult);
    if (n) HIP_TRY(hipMemcpyAsync(out, b->d_out + item_begin, n, hipMemcpyDeviceToHost, st));
    svtgpu_count_xfer(1, n);
    HIP_TRY(hipStreamSynchronize(st));
    return SVTGPU_OK;
}
