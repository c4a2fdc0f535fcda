/*
 * gen_golden_obmc.c — writes tests/golden/obmc.bin: the reference's own OBMC distortion kernels and full-pel OBMC
 * search on deterministic inputs (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C, compiled straight from its tree (REF = the reference checkout, run from the
 * repository root; the binary goes outside the repository):
 *
 *   S=$REF/Source; gcc -O2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w \
 *     -I$S/API -I$S/Lib/Common/Codec -I$S/Lib/Common/C_DEFAULT -I$S/Lib/Encoder/Codec -I$S/Lib/Encoder/C_DEFAULT \
 *     -I$S/Lib/Encoder/Globals -I$S/Lib/Common/ASM_AVX2 -I$S/Lib/Encoder/ASM_AVX2 -I$S/Lib/Common/ASM_SSE2 \
 *     -I$S/Lib/Common/ASM_SSE4_1 -I$REF/third_party/aom/inc -I$REF/third_party/cpuinfo/include -I$REF \
 *     -Ioracle/ref_harness tests/golden/gen_golden_obmc.c $S/Lib/Encoder/C_DEFAULT/sad_av1.c \
 *     $S/Lib/Encoder/C_DEFAULT/variance.c $S/Lib/Encoder/Codec/av1me.c $S/Lib/Encoder/Codec/EbRateDistortionCost.c \
 *     -o /tmp/gen_golden_obmc -Wl,--gc-sections -lm
 *   /tmp/gen_golden_obmc tests/golden/obmc.bin
 *   /tmp/gen_golden_obmc --time            # the perf workload of scripts/obmc_perf.py through the C walk, one core
 *
 * Records (golden_io format; tests/obmc_cases.py reads them):
 *   sizes                 i32 [22][2]   {W, H} in the order of the blk records
 *   blk<k>_pre            u8  [2][(H + 1) * (W + 1)]   pre windows (stride W + 1) of the random and the boundary case
 *   blk<k>_wsrc           i32 [2][W * H]
 *   blk<k>_mask           u16 [2][W * H]
 *   blk<k>_res            u32 [4][11]   per case {sad, var, sse, (var, sse) at sub-pel (0,0), (4,4), (7,3), (0,5)}:
 *                         case 0 random (pre u8, mask in [0, 4096], wsrc in [0, 255 * 4096]); case 1 boundary (wsrc -
 *                         pre * mask within +-1 of +-2048 + k * 4096); case 2 wsrc = 255 * 4096, mask = 0, pre of
 *                         case 0 (every diff +255); case 3 wsrc = 0, mask = 4096, pre = 255 (every diff -255)
 *   walk_frames           u8  [3][FH][FW]  reference pictures: smooth noise, a horizontal ramp, flat
 *   walk<i>_par           i32 [18]      {frame, x, y, w, h, mvp_col, mvp_row, ref_mv_col, ref_mv_row, col_min, col_max,
 *                                        row_min, row_max, sad_per_bit, search_range, search_diag, cost_mode,
 *                                        errorperbit}
 *   walk<i>_wsrc / _mask  i32 / u16 [w * h]
 *   walk<i>_cost          i32 [4 + 2 * (2 * range + 1)]  the batch's cost tables (include/svtgpu.h), cost_mode 1 only
 *   walk<i>_res           i32 [5]       {dst_mv col, row, ovf at dst_mv, its sse, svt_av1_obmc_full_pixel_search's
 *                                        return}
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbModeDecisionProcess.h"
#include "av1me.h"
#include "mcomp.h"
#include "golden_io.h"

int svt_av1_obmc_full_pixel_search(ModeDecisionContext *ctx, IntraBcContext *x, MV *mvp_full, int sadpb,
                                   const AomVarianceFnPtr *fn_ptr, const MV *ref_mv, MV *dst_mv, int is_second);

#define FOR_SIZES(X)                                                                                               \
    X(4, 4) X(4, 8) X(8, 4) X(8, 8) X(8, 16) X(16, 8) X(16, 16) X(16, 32) X(32, 16) X(32, 32) X(32, 64) X(64, 32) \
    X(64, 64) X(64, 128) X(128, 64) X(128, 128) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)

#define DECL(W, H)                                                                                                 \
    unsigned int svt_aom_obmc_sad##W##x##H##_c(const uint8_t *, int, const int32_t *, const int32_t *);            \
    unsigned int svt_aom_obmc_variance##W##x##H##_c(const uint8_t *, int, const int32_t *, const int32_t *,       \
                                                    unsigned int *);                                               \
    unsigned int svt_aom_obmc_sub_pixel_variance##W##x##H##_c(const uint8_t *, int, int, int, const int32_t *,    \
                                                              const int32_t *, unsigned int *);
FOR_SIZES(DECL)

typedef struct SizeFns {
    int                     w, h;
    AomObmcSadFn            osdf;
    AomObmcVarianceFn       ovf;
    AomObmcSubpixvarianceFn osvf;
} SizeFns;
#define ENTRY(W, H) \
    {W, H, svt_aom_obmc_sad##W##x##H##_c, svt_aom_obmc_variance##W##x##H##_c, svt_aom_obmc_sub_pixel_variance##W##x##H##_c},
static const SizeFns kSizes[22] = {FOR_SIZES(ENTRY)};

static const SizeFns *size_fns(int w, int h) {
    for (int k = 0; k < 22; k++)
        if (kSizes[k].w == w && kSizes[k].h == h) return &kSizes[k];
    fprintf(stderr, "no size %dx%d\n", w, h);
    exit(2);
}

static const int kSub[4][2] = {{0, 0}, {4, 4}, {7, 3}, {0, 5}}; /* {xoffset, yoffset} */
#define WSRC_MAX (255 * 4096)

static void block_results(const SizeFns *f, const uint8_t *pre, const int32_t *wsrc, const int32_t *mask,
                          uint32_t *res) {
    const int ps = f->w + 1;
    unsigned  sse;
    res[0] = f->osdf(pre, ps, wsrc, mask);
    res[1] = f->ovf(pre, ps, wsrc, mask, &sse);
    res[2] = sse;
    for (int s = 0; s < 4; s++) {
        res[3 + 2 * s] = f->osvf(pre, ps, kSub[s][0], kSub[s][1], wsrc, mask, &sse);
        res[4 + 2 * s] = sse;
    }
}

static void block_cases(GoldenFile *g, Rng *rng) {
    int32_t dims[22][2];
    for (int k = 0; k < 22; k++) dims[k][0] = kSizes[k].w, dims[k][1] = kSizes[k].h;
    golden_put2(g, "sizes", 'i', 22, 2, dims);
    for (int k = 0; k < 22; k++) {
        const SizeFns *f = &kSizes[k];
        const int      w = f->w, h = f->h, n = w * h, pn = (h + 1) * (w + 1);
        uint8_t       *pre  = malloc(2 * pn);
        int32_t       *wsrc = malloc(2 * n * sizeof(int32_t)), *mask = malloc(2 * n * sizeof(int32_t));
        uint16_t      *m16  = malloc(2 * n * sizeof(uint16_t));
        uint32_t       res[4][11];
        for (int i = 0; i < 2 * pn; i++) pre[i] = (uint8_t)rng_below(rng, 256);
        for (int i = 0; i < n; i++) { /* case 0: random */
            mask[i] = (int32_t)rng_below(rng, 4097);
            wsrc[i] = (int32_t)rng_below(rng, WSRC_MAX + 1);
        }
        for (int i = 0; i < n; i++) { /* case 1: the rounding boundary of the sample the full-pel kernels read */
            const int     p = pre[pn + (i / w) * (w + 1) + i % w];
            const int32_t m = (int32_t)rng_below(rng, 4097);
            int32_t       t = 2048 + 4096 * (int32_t)rng_below(rng, 60) + (int32_t)rng_below(rng, 3) - 1;
            if (rng_below(rng, 2)) t = -t;
            if (p * m + t < 0 || p * m + t > WSRC_MAX) t = -t;
            if (p * m + t < 0 || p * m + t > WSRC_MAX) t = t < 0 ? -2048 - (t & 1) : 2048 + (t & 1);
            if (p * m + t < 0 || p * m + t > WSRC_MAX) t = -t;
            mask[n + i] = m;
            wsrc[n + i] = p * m + t;
        }
        block_results(f, pre, wsrc, mask, res[0]);
        block_results(f, pre + pn, wsrc + n, mask + n, res[1]);
        {
            int32_t *cw = malloc(n * sizeof(int32_t)), *cm = malloc(n * sizeof(int32_t));
            uint8_t *cp = malloc(pn);
            for (int i = 0; i < n; i++) cw[i] = WSRC_MAX, cm[i] = 0;
            block_results(f, pre, cw, cm, res[2]);
            for (int i = 0; i < n; i++) cw[i] = 0, cm[i] = 4096;
            memset(cp, 255, pn);
            block_results(f, cp, cw, cm, res[3]);
            free(cw), free(cm), free(cp);
        }
        for (int i = 0; i < 2 * n; i++) m16[i] = (uint16_t)mask[i];
        char name[64];
        snprintf(name, sizeof name, "blk%d_pre", k);
        golden_put2(g, name, 'B', 2, pn, pre);
        snprintf(name, sizeof name, "blk%d_wsrc", k);
        golden_put2(g, name, 'i', 2, n, wsrc);
        snprintf(name, sizeof name, "blk%d_mask", k);
        golden_put2(g, name, 'H', 2, n, m16);
        snprintf(name, sizeof name, "blk%d_res", k);
        golden_put2(g, name, 'I', 4, 11, res);
        free(pre), free(wsrc), free(mask), free(m16);
    }
}

/* ---- the walk: the reference's svt_av1_obmc_full_pixel_search on a padded picture ---- */
#define PAD 192
#define TAB 16384 /* MV_UPP: the cost tables cover [-TAB, TAB] */

typedef struct Picture {
    int      w, h, stride;
    uint8_t *buf; /* padded by edge replication, as the encoder's reference pictures */
} Picture;

static uint8_t *pic_at(const Picture *p, int x, int y) { return p->buf + (size_t)(y + PAD) * p->stride + x + PAD; }

static Picture make_picture(int w, int h, const uint8_t *px) {
    Picture p = {w, h, w + 2 * PAD, NULL};
    p.buf     = malloc((size_t)p.stride * (h + 2 * PAD));
    for (int y = -PAD; y < h + PAD; y++)
        for (int x = -PAD; x < w + PAD; x++) {
            const int cy = y < 0 ? 0 : y >= h ? h - 1 : y, cx = x < 0 ? 0 : x >= w ? w - 1 : x;
            *pic_at(&p, x, y) = px[cy * w + cx];
        }
    return p;
}

typedef struct Walk {
    int frame, x, y, w, h, mvp_col, mvp_row, ref_mv_col, ref_mv_row, col_min, col_max, row_min, row_max, sad_per_bit,
        range, diag, cost_mode, errorperbit;
} Walk;

static int  g_joint[4] = {310, 1187, 1243, 1920};
static int *g_comp[2]; /* centred tables */

static void make_cost_tables(void) {
    for (int c = 0; c < 2; c++) {
        int *t = malloc((2 * TAB + 1) * sizeof(int));
        for (int v = -TAB; v <= TAB; v++) {
            const unsigned a = (unsigned)(v < 0 ? -v : v);
            int            bits = 0;
            while ((a >> bits) > 0) bits++;
            t[v + TAB] = 420 + 290 * bits + (int)((a * 2654435761u + (unsigned)c * 97u) >> 27) + (v < 0 ? 37 : 0);
        }
        g_comp[c] = t + TAB;
    }
}

static int clip_tab(int v) { return v < -TAB ? -TAB : v > TAB ? TAB : v; }

/* one call of the reference's search; res = {col, row, ovf, sse, return} */
static void run_walk(const Walk *k, const Picture *pic, const int32_t *wsrc, const int32_t *mask,
                     ModeDecisionContext *ctx, IntraBcContext *x, int32_t *res) {
    const SizeFns   *f = size_fns(k->w, k->h);
    AomVarianceFnPtr fn;
    memset(&fn, 0, sizeof fn);
    fn.osdf = f->osdf, fn.ovf = f->ovf, fn.osvf = f->osvf;
    memset(x, 0, sizeof *x);
    ctx->wsrc_buf                     = (int32_t *)wsrc;
    ctx->mask_buf                     = (int32_t *)mask;
    ctx->obmc_ctrls.fpel_search_range = (uint8_t)k->range;
    ctx->obmc_ctrls.fpel_search_diag  = (uint8_t)k->diag;
    ctx->approx_inter_rate            = k->cost_mode == 0;
    x->xdplane[0].pre[0].buf          = pic_at(pic, k->x, k->y);
    x->xdplane[0].pre[0].stride       = pic->stride;
    x->mv_limits.col_min = k->col_min, x->mv_limits.col_max = k->col_max;
    x->mv_limits.row_min = k->row_min, x->mv_limits.row_max = k->row_max;
    x->nmv_vec_cost  = g_joint;
    x->mv_cost_stack = g_comp;
    x->errorperbit   = k->errorperbit;
    MV mvp = {(int16_t)k->mvp_row, (int16_t)k->mvp_col}, ref = {(int16_t)k->ref_mv_row, (int16_t)k->ref_mv_col}, dst;
    const int ret = svt_av1_obmc_full_pixel_search(ctx, x, &mvp, k->sad_per_bit, &fn, &ref, &dst, 0);
    unsigned  sse;
    res[0] = dst.col, res[1] = dst.row;
    res[2] = (int32_t)f->ovf(pic_at(pic, k->x + dst.col, k->y + dst.row), pic->stride, wsrc, mask, &sse);
    res[3] = (int32_t)sse;
    res[4] = ret;
}

#define FW 96
#define FH 64

/* wsrc = mask * (the picture displaced by (tx, ty)) + noise: the SAD landscape has its minimum near that MV */
static void make_target(const Picture *pic, const Walk *k, int tx, int ty, int flat_mask, int noise, Rng *rng,
                        int32_t *wsrc, int32_t *mask) {
    for (int py = 0; py < k->h; py++)
        for (int px = 0; px < k->w; px++) {
            const int m = flat_mask ? 4096 : 1024 + (int)rng_below(rng, 3073);
            int       v = *pic_at(pic, k->x + px + tx, k->y + py + ty) * m;
            if (noise) v += (int)rng_below(rng, 2 * noise + 1) - noise;
            mask[py * k->w + px] = m;
            wsrc[py * k->w + px] = v < 0 ? 0 : v > WSRC_MAX ? WSRC_MAX : v;
        }
}

static void walk_cases(GoldenFile *g, Rng *rng) {
    static uint8_t frames[3][FH][FW];
    /* 0: smooth noise (a random walk in both directions); 1: a horizontal ramp; 2: flat */
    for (int y = 0; y < FH; y++)
        for (int x = 0; x < FW; x++) {
            const int a = x ? frames[0][y][x - 1] : 128, b = y ? frames[0][y - 1][x] : a;
            int       v = (a + b) / 2 + (int)rng_below(rng, 25) - 12;
            frames[0][y][x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            frames[1][y][x] = (uint8_t)(2 * x + 8);
            frames[2][y][x] = 77;
        }
    uint32_t fd[3] = {3, FH, FW};
    golden_put(g, "walk_frames", 'B', 3, fd, frames);
    Picture pics[3];
    for (int i = 0; i < 3; i++) pics[i] = make_picture(FW, FH, &frames[i][0][0]);
    ModeDecisionContext *ctx = calloc(1, sizeof *ctx);
    IntraBcContext      *x   = calloc(1, sizeof *x);

    /* {walk, target displacement tx, ty, flat mask, noise} */
    struct {
        Walk k;
        int  tx, ty, flat, noise;
    } cs[] = {
        /* smooth noise, both cost modes, both range / diag settings */
        {{0, 40, 24, 16, 16, 0, 0, 0, 0, -60, 60, -60, 60, 60, 16, 1, 0, 110}, 5, -3, 0, 900},
        {{0, 40, 24, 16, 16, 0, 0, 0, 0, -60, 60, -60, 60, 60, 8, 0, 0, 110}, 5, -3, 0, 900},
        {{0, 40, 24, 16, 16, 1, 2, 11, -21, -60, 60, -60, 60, 45, 16, 1, 1, 150}, -4, 6, 0, 900},
        {{0, 40, 24, 16, 16, 1, 2, 11, -21, -60, 60, -60, 60, 45, 8, 0, 1, 150}, -4, 6, 0, 900},
        {{0, 8, 8, 8, 8, -2, 3, -16, 24, -30, 30, -30, 30, 80, 16, 1, 1, 90}, 3, 3, 0, 400},
        {{0, 60, 40, 32, 16, 4, -4, 30, -30, -40, 40, -40, 40, 30, 16, 1, 0, 90}, 9, 1, 0, 2000},
        {{0, 16, 0, 64, 64, 0, 0, 0, 0, -40, 40, -40, 40, 25, 16, 1, 1, 60}, -6, 7, 0, 3000},
        {{0, 0, 44, 4, 16, 2, 2, 8, 8, -20, 20, -20, 20, 70, 8, 0, 1, 60}, 0, -5, 0, 300},
        /* blocks whose window leaves the picture on each side */
        {{0, 0, 0, 16, 16, -3, -2, -20, -10, -50, 50, -50, 50, 50, 16, 1, 0, 80}, -7, -6, 0, 500},
        {{0, 80, 48, 16, 16, 3, 2, 20, 10, -50, 50, -50, 50, 50, 16, 1, 1, 80}, 8, 7, 0, 500},
        /* a start outside the limits, which gets clamped */
        {{0, 40, 24, 16, 16, 25, -30, 40, -40, -10, 12, -9, 14, 60, 16, 1, 0, 110}, 5, -3, 0, 900},
        {{0, 40, 24, 16, 16, -25, 30, -40, 40, -10, 12, -9, 14, 60, 8, 0, 1, 110}, 5, -3, 0, 900},
        /* limits that cut the walk: the ramp's minimum lies 20 columns away, col_max stops it after 5 */
        {{1, 24, 16, 16, 16, 0, 0, 0, 0, -60, 5, -60, 60, 20, 16, 1, 0, 100}, 20, 0, 1, 0},
        {{1, 24, 16, 16, 16, 0, 0, 0, 0, -60, 5, -60, 60, 4, 16, 0, 1, 100}, 20, 0, 1, 0},
        /* a monotone gradient that runs the full range (16 with diagonals, 8 without) */
        {{1, 24, 16, 16, 16, 0, 0, 0, 0, -60, 60, -60, 60, 20, 16, 1, 0, 100}, 20, 0, 1, 0},
        {{1, 24, 16, 16, 16, 0, 0, 0, 0, -60, 60, -60, 60, 4, 8, 0, 1, 100}, -20, 0, 1, 0},
        /* a walk that stops at step 0: the start is the minimum */
        {{0, 40, 24, 16, 16, 5, -3, 40, -24, -60, 60, -60, 60, 60, 16, 1, 0, 110}, 5, -3, 1, 0},
        {{0, 40, 24, 8, 8, 5, -3, 40, -24, -60, 60, -60, 60, 60, 8, 0, 1, 110}, 5, -3, 1, 0},
        /* flat content: every candidate's SAD ties and nothing may be taken */
        {{2, 40, 24, 16, 16, 2, 1, 16, 8, -60, 60, -60, 60, 60, 16, 1, 0, 110}, 0, 0, 0, 700},
        {{2, 40, 24, 16, 16, 2, 1, 16, 8, -60, 60, -60, 60, 60, 16, 1, 1, 110}, 0, 0, 0, 700},
        /* search_range 0: the start alone */
        {{0, 40, 24, 16, 16, 1, 1, 0, 0, -60, 60, -60, 60, 60, 0, 1, 0, 110}, 5, -3, 0, 900},
    };
    const int ncase = (int)(sizeof cs / sizeof cs[0]);
    int32_t   nc    = ncase;
    golden_put1(g, "walk_count", 'i', 1, &nc);
    for (int i = 0; i < ncase; i++) {
        const Walk *k = &cs[i].k;
        const int   n = k->w * k->h, T = 2 * k->range + 1;
        int32_t    *wsrc = malloc(n * sizeof(int32_t)), *mask = malloc(n * sizeof(int32_t));
        uint16_t   *m16 = malloc(n * sizeof(uint16_t));
        int32_t     res[5], par[18];
        make_target(&pics[k->frame], k, cs[i].tx, cs[i].ty, cs[i].flat, cs[i].noise, rng, wsrc, mask);
        run_walk(k, &pics[k->frame], wsrc, mask, ctx, x, res);
        memcpy(par, k, sizeof par);
        for (int j = 0; j < n; j++) m16[j] = (uint16_t)mask[j];
        char name[64];
        snprintf(name, sizeof name, "walk%d_par", i);
        golden_put1(g, name, 'i', 18, par);
        snprintf(name, sizeof name, "walk%d_wsrc", i);
        golden_put1(g, name, 'i', n, wsrc);
        snprintf(name, sizeof name, "walk%d_mask", i);
        golden_put1(g, name, 'H', n, m16);
        if (k->cost_mode == 1) { /* the tables the batch takes (include/svtgpu.h) */
            int32_t  *tab = malloc((4 + 2 * T) * sizeof(int32_t));
            const int sr = k->mvp_row < k->row_min ? k->row_min : k->mvp_row > k->row_max ? k->row_max : k->mvp_row;
            const int sc = k->mvp_col < k->col_min ? k->col_min : k->mvp_col > k->col_max ? k->col_max : k->mvp_col;
            for (int j = 0; j < 4; j++) tab[j] = g_joint[j];
            for (int j = 0; j < T; j++) {
                tab[4 + j]     = g_comp[0][clip_tab((sr - k->range + j - (k->ref_mv_row >> 3)) * 8)];
                tab[4 + T + j] = g_comp[1][clip_tab((sc - k->range + j - (k->ref_mv_col >> 3)) * 8)];
            }
            snprintf(name, sizeof name, "walk%d_cost", i);
            golden_put1(g, name, 'i', 4 + 2 * T, tab);
            free(tab);
        }
        snprintf(name, sizeof name, "walk%d_res", i);
        golden_put1(g, name, 'i', 5, res);
        free(wsrc), free(mask), free(m16);
    }
}

/* ---- --time: the workload of scripts/obmc_perf.py (every 16x16 block of a 1920x1080 picture, range 16 with
 * diagonals, cost mode 0) through the reference's C walk on this core ---- */
static int tri(int v) {
    const int t = 2 * abs((v & 255) - 128);
    return t > 255 ? 255 : t;
}
static void time_mode(void) {
    const int W = 1920, H = 1080, bw = 16, bh = 16, nbx = W / bw, nby = H / bh, n = bw * bh;
    uint8_t  *px = malloc((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) px[(size_t)y * W + x] = (uint8_t)((tri(3 * x + y) + tri(5 * y - x + 1000)) >> 1);
    Picture              pic  = make_picture(W, H, px);
    int32_t             *wsrc = malloc((size_t)nbx * nby * n * sizeof(int32_t)), *mask = malloc(n * sizeof(int32_t));
    ModeDecisionContext *ctx  = calloc(1, sizeof *ctx);
    IntraBcContext      *x    = calloc(1, sizeof *x);
    for (int py = 0; py < bh; py++)
        for (int qx = 0; qx < bw; qx++) mask[py * bw + qx] = 2048 + 64 * (qx + py);
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            const int dx = (bx * 7 + by * 3) % 25 - 12, dy = (bx * 5 + by * 11) % 25 - 12;
            int32_t  *w  = wsrc + (size_t)(by * nbx + bx) * n;
            for (int py = 0; py < bh; py++)
                for (int qx = 0; qx < bw; qx++)
                    w[py * bw + qx] = mask[py * bw + qx] * *pic_at(&pic, bx * bw + qx + dx, by * bh + py + dy);
        }
    long long       steps = 0, check = 0;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            const Walk k = {0, bx * bw, by * bh, bw, bh, 0, 0, 0, 0, -64, 64, -64, 64, 60, 16, 1, 0, 100};
            int32_t    res[5];
            run_walk(&k, &pic, wsrc + (size_t)(by * nbx + bx) * n, mask, ctx, x, res);
            steps += abs(res[0]) > abs(res[1]) ? abs(res[0]) : abs(res[1]);
            check += res[2] + 3 * res[0] + 7 * res[1];
        }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
    printf("{\"workload\": \"1920x1080 8-bit, every 16x16 block, range 16 with diagonals, cost mode 0\", "
           "\"items\": %d, \"ms\": %.3f, \"items_per_s\": %.0f, \"chebyshev_moves\": %lld, \"checksum\": %lld}\n",
           nbx * nby, ms, nbx * nby / (ms * 1e-3), steps, check);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <obmc.bin> | --time\n", argv[0]);
        return 2;
    }
    make_cost_tables();
    if (!strcmp(argv[1], "--time")) {
        time_mode();
        return 0;
    }
    Rng        rng = {0x0B3C5EEDull};
    GoldenFile g   = golden_open(argv[1]);
    block_cases(&g, &rng);
    walk_cases(&g, &rng);
    golden_close(&g);
    return 0;
}
