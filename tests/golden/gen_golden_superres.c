/*
 * gen_golden_superres.c — writes tests/golden/superres.bin: the reference's own normative super-resolution upscale,
 * and its loop restoration of super-resolved frames, on deterministic inputs (test infrastructure; never shipped, not
 * built by build()).
 *
 * It links the REFERENCE's C, compiled straight from its tree (REF = the reference checkout, run from the
 * repository root; the binary goes outside the repository).  EbSuperRes.c is included below, not linked: the step,
 * start-phase and scaled-size helpers are static or undeclared there.
 *
 *   S=$REF/Source; C=$S/Lib/Common/Codec; gcc -O2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w \
 *     -I$S/API -I$C -I$S/Lib/Common/C_DEFAULT -I$S/Lib/Encoder/Codec -I$S/Lib/Encoder/C_DEFAULT \
 *     -I$S/Lib/Encoder/Globals -I$S/Lib/Common/ASM_AVX2 -I$S/Lib/Encoder/ASM_AVX2 -I$S/Lib/Common/ASM_SSE2 \
 *     -I$S/Lib/Common/ASM_SSE4_1 -I$REF/third_party/aom/inc -I$REF/third_party/cpuinfo/include -I$REF \
 *     -Ioracle/ref_harness tests/golden/gen_golden_superres.c $C/convolve.c $C/EbRestoration.c \
 *     $C/EbCdef.c $C/EbPictureBufferDesc.c $C/EbMalloc.c $C/EbLog.c $C/EbThreads.c $C/EbBlockStructures.c \
 *     $C/EbPictureOperators.c $C/common_dsp_rtcd.c $C/EbUtility.c $S/Lib/Common/C_DEFAULT/EbPictureOperators_C.c \
 *     $S/Lib/Encoder/Codec/aom_dsp_rtcd.c -o /tmp/gen_golden_superres -Wl,--gc-sections -lm -lpthread
 *   /tmp/gen_golden_superres tests/golden/superres.bin
 *   /tmp/gen_golden_superres --time     # scripts/superres_perf.py's workload through the reference's C, one core
 *
 * Records (golden_io format; tests/superres_cases.py reads them):
 *   filter            i16 [64][8]   av1_resize_filter_normative
 *   scaled_dims       i32 [6]       the dims of `scaled`
 *   scaled            i32 [6][10]   calculate_scaled_size_helper(dim, denom), denom = 8..17
 *   nup               i32 [1]       upscale records
 *   up<i>_par         i32 [10]      {bit_depth, sub_x, frame_width, upscaled_width, denominator, rows, in_w, out_w,
 *                                    coded plane width, tile columns the reference ran with}
 *   up<i>_src         u16 [rows][coded plane width]   one plane of the downscaled picture (the columns between in_w and
 *                                    the coded width are random or the pattern's continuation: the taps read them)
 *   up<i>_out         u16 [rows][out_w]               svt_av1_upscale_normative_rows of it
 *   geom              i32 [nup][4]  {in_w, out_w, av1_get_upscale_convolve_step, get_upscale_convolve_x0}
 *   nlr               i32 [1]       loop-restoration cases
 *   lr<i>_params      i32 [7]       {upscaled_width, height, bit_depth, luma unit size, planes restored (bit mask),
 *                                    frame_width, denominator}
 *   lr<i>_dlf<p> / lr<i>_cdef<p>    u8 / u16 [plane rows][coded plane width]   the downscaled deblocked / CDEF frames
 *   lr<i>_units<p>    i32 [units][20]   as lr_frame.bin's c<i>_units<p>
 *   lr<i>_out<p>      u8 / u16 [plane rows][upscaled plane width]   svt_av1_loop_restoration_filter_frame of the
 *                                    upscaled CDEF frame with the boundary lines the reference saved before it
 *
 * The upscale cases: every denominator 9..16 at upscaled 88x16, 8- and 10-bit, luma and chroma; an odd upscaled width
 * (83, chroma 42) and a downscaled crop width that is no multiple of 8 (352 -> 313, coded 320); extreme content
 * (rows of alternating 0 / max columns in both phases, max-valued impulses, flat max, 0 / max column pairs and zero
 * dips in flat max: sums below 0 and above max before the clip); one two-tile-column picture
 * (208 -> 139, coded 144, tile_col_start_mi {0, 16, 36}) run with two tile columns and with one -- the generator
 * stops unless the two outputs are equal -- and two rows of 1920 -> 3840, 10-bit.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbRestoration.h"
#include "EbPictureControlSet.h"
#include "Av1Common.h"
#include "common_dsp_rtcd.h"
#include "aom_dsp_rtcd.h"
#include "EbCodingUnit.h"
#include "EbThreads.h"
#include "golden_io.h"

#include "EbSuperRes.c"

void    svt_av1_loop_restoration_filter_frame(int32_t *rst_tmpbuf, Yv12BufferConfig *frame, Av1Common *cm,
                                              int32_t optimized_lr);
void    svt_av1_loop_restoration_save_boundary_lines(const Yv12BufferConfig *frame, Av1Common *cm, int32_t after_cdef);
int32_t svt_aom_realloc_frame_buffer(Yv12BufferConfig *ybf, int32_t width, int32_t height, int32_t ss_x, int32_t ss_y,
                                     int32_t use_highbitdepth, int32_t border, int32_t byte_alignment,
                                     AomCodecFrameBuffer *fb, AomGetFrameBufferCbFn cb, void *cb_priv);
EbErrorType svt_av1_alloc_restoration_buffers(PictureControlSet *pcs, Av1Common *cm);

static void bind_c_kernels(void) {
    svt_av1_wiener_convolve_add_src        = svt_av1_wiener_convolve_add_src_c;
    svt_av1_highbd_wiener_convolve_add_src = svt_av1_highbd_wiener_convolve_add_src_c;
    svt_av1_selfguided_restoration         = svt_av1_selfguided_restoration_c;
    svt_apply_selfguided_restoration       = svt_apply_selfguided_restoration_c;
    svt_memcpy                             = svt_memcpy_c;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
static int scaled(int dim, int denom) {
    uint16_t d = (uint16_t)dim;
    calculate_scaled_size_helper(&d, (uint8_t)denom);
    return d;
}

/* the superres fields of an Av1Common: one tile column unless tile_starts is given */
static void set_superres(Av1Common *cm, int frame_width, int upscaled_width, int denom, int ntile,
                         const int *tile_starts) {
    cm->frm_size.frame_width             = (uint16_t)frame_width;
    cm->frm_size.superres_upscaled_width = (uint16_t)upscaled_width;
    cm->frm_size.superres_denominator    = (uint8_t)denom;
    cm->mi_cols                          = ((frame_width + 7) & ~7) >> 2;
    cm->tiles_info.tile_cols             = (uint8_t)ntile;
    for (int j = 0; j <= ntile; j++)
        cm->tiles_info.tile_col_start_mi[j] = (uint16_t)(tile_starts ? tile_starts[j] : j ? cm->mi_cols : 0);
}

/* ---- plane-level upscale records ---- */
enum { CONTENT_RANDOM, CONTENT_EXTREME };
typedef struct UpCase {
    int bd, sub_x, upscaled_width, denom, rows, content, ntile;
    int tile_starts[3];
} UpCase;

#define BORDER 16 /* the reference writes (and restores) 5 columns either side of the coded width */

static void run_plane(const UpCase *c, int ntile, const uint16_t *src, int coded, uint16_t *out, int out_w) {
    Av1Common *cm = calloc(1, sizeof(Av1Common));
    set_superres(cm, scaled(c->upscaled_width, c->denom), c->upscaled_width, c->denom, ntile,
                 ntile > 1 ? c->tile_starts : NULL);
    const int hb = c->bd > 8, ss = coded + 2 * BORDER, ds = out_w + 2 * BORDER, bs = hb ? 2 : 1;
    uint8_t  *s = calloc((size_t)c->rows * ss, bs), *d = calloc((size_t)c->rows * ds, bs);
    for (int y = 0; y < c->rows; y++)
        for (int x = 0; x < coded; x++) {
            if (hb)
                ((uint16_t *)s)[y * ss + BORDER + x] = src[y * coded + x];
            else
                s[y * ss + BORDER + x] = (uint8_t)src[y * coded + x];
        }
    svt_av1_upscale_normative_rows(cm, s + BORDER * bs, ss, d + BORDER * bs, ds, c->rows, c->sub_x, c->bd, hb);
    for (int y = 0; y < c->rows; y++)
        for (int x = 0; x < out_w; x++)
            out[y * out_w + x] = hb ? ((uint16_t *)d)[y * ds + BORDER + x] : d[y * ds + BORDER + x];
    free(s), free(d), free(cm);
}

static void fill_plane(const UpCase *c, Rng *r, uint16_t *src, int coded, int in_w) {
    const int maxv = (1 << c->bd) - 1;
    for (int y = 0; y < c->rows; y++)
        for (int x = 0; x < coded; x++) {
            int v;
            if (c->content == CONTENT_RANDOM)
                v = y & 1 ? (int)rng_below(r, (uint32_t)maxv + 1)
                          : clampi((x * 5 + y * 3) * (maxv + 1) / 512 + (int)rng_below(r, (uint32_t)(maxv / 4 + 1)), 0, maxv);
            else if (y % 6 == 0)
                v = x & 1 ? maxv : 0;
            else if (y % 6 == 1)
                v = x & 1 ? 0 : maxv;
            else if (y % 6 == 2 || y % 6 == 5) { /* max-valued impulses; row 5: zero dips in flat max */
                v = (x == 0 || x == 1 || x == 20 || x == in_w / 2 || x == in_w - 1 || x == coded - 1) ? maxv : 0;
                if (y % 6 == 5) v = maxv - v;
            } else if (y % 6 == 3)
                v = maxv;
            else
                v = x & 2 ? 0 : maxv; /* pairs: both positive centre taps on max, their negative neighbours on 0 */
            src[y * coded + x] = (uint16_t)v;
        }
}

static void gen_upscale(GoldenFile *g) {
    static UpCase cases[80];
    int           n = 0;
    for (int bd = 8; bd <= 10; bd += 2)
        for (int sub_x = 0; sub_x < 2; sub_x++)
            for (int denom = 9; denom <= 16; denom++)
                cases[n++] = (UpCase){bd, sub_x, 88, denom, sub_x ? 8 : 16, CONTENT_RANDOM, 1, {0}};
    for (int bd = 8; bd <= 10; bd += 2)
        for (int sub_x = 0; sub_x < 2; sub_x++) {
            cases[n++] = (UpCase){bd, sub_x, 83, 11, 4, CONTENT_RANDOM, 1, {0}};
            cases[n++] = (UpCase){bd, sub_x, 83, 16, 4, CONTENT_RANDOM, 1, {0}};
            cases[n++] = (UpCase){bd, sub_x, 352, 9, 4, CONTENT_RANDOM, 1, {0}};
        }
    for (int bd = 8; bd <= 10; bd += 2) {
        cases[n++] = (UpCase){bd, 0, 88, 13, 12, CONTENT_EXTREME, 1, {0}};
        cases[n++] = (UpCase){bd, 0, 88, 16, 6, CONTENT_EXTREME, 1, {0}};
        cases[n++] = (UpCase){bd, 1, 83, 10, 6, CONTENT_EXTREME, 1, {0}};
    }
    for (int sub_x = 0; sub_x < 2; sub_x++) cases[n++] = (UpCase){10, sub_x, 208, 12, 4, CONTENT_RANDOM, 2, {0, 16, 36}};
    cases[n++] = (UpCase){8, 0, 208, 12, 6, CONTENT_EXTREME, 2, {0, 16, 36}};
    cases[n++] = (UpCase){10, 0, 3840, 16, 2, CONTENT_RANDOM, 1, {0}};

    Rng      r    = {0x5352000000000001ull};
    int32_t  nup  = n;
    int32_t *geom = calloc((size_t)n, 4 * sizeof(int32_t));
    golden_put1(g, "nup", 'i', 1, &nup);
    for (int i = 0; i < n; i++) {
        const UpCase *c  = &cases[i];
        const int     fw = scaled(c->upscaled_width, c->denom);
        const int     in_w = (fw + c->sub_x) >> c->sub_x, out_w = (c->upscaled_width + c->sub_x) >> c->sub_x;
        const int     coded = ((fw + 7) & ~7) >> c->sub_x;
        uint16_t     *src = malloc(sizeof(uint16_t) * c->rows * coded);
        uint16_t     *out = malloc(sizeof(uint16_t) * c->rows * out_w), *out1 = malloc(sizeof(uint16_t) * c->rows * out_w);
        fill_plane(c, &r, src, coded, in_w);
        run_plane(c, c->ntile, src, coded, out, out_w);
        if (c->ntile > 1) { /* the same picture as one tile column: the device entry takes no tile information */
            run_plane(c, 1, src, coded, out1, out_w);
            if (memcmp(out, out1, sizeof(uint16_t) * c->rows * out_w)) {
                fprintf(stderr, "case %d: %d tile columns and one give different outputs\n", i, c->ntile);
                exit(3);
            }
        }
        int32_t par[10] = {c->bd, c->sub_x, fw, c->upscaled_width, c->denom, c->rows, in_w, out_w, coded, c->ntile};
        char    nm[32];
        snprintf(nm, sizeof nm, "up%d_par", i);
        golden_put1(g, nm, 'i', 10, par);
        snprintf(nm, sizeof nm, "up%d_src", i);
        golden_put2(g, nm, 'H', (uint32_t)c->rows, (uint32_t)coded, src);
        snprintf(nm, sizeof nm, "up%d_out", i);
        golden_put2(g, nm, 'H', (uint32_t)c->rows, (uint32_t)out_w, out);
        int32_t *e = geom + 4 * i;
        e[0] = in_w, e[1] = out_w, e[2] = av1_get_upscale_convolve_step(in_w, out_w);
        e[3] = get_upscale_convolve_x0(in_w, out_w, e[2]);
        free(src), free(out), free(out1);
    }
    golden_put2(g, "geom", 'i', (uint32_t)n, 4, geom);
    free(geom);
}

static void gen_scaled(GoldenFile *g) {
    static const int32_t dims[6] = {8, 15, 16, 17, 352, 3840};
    int32_t              v[6][10];
    for (int i = 0; i < 6; i++)
        for (int d = 8; d <= 17; d++) v[i][d - 8] = scaled(dims[i], d);
    golden_put1(g, "scaled_dims", 'i', 6, dims);
    golden_put2(g, "scaled", 'i', 6, 10, v);
    golden_put2(g, "filter", 'h', 64, 8, av1_resize_filter_normative);
}

/* ---- loop restoration of super-resolved frames (the way gen_golden_lr.c's gen_frames builds lr_frame.bin) ---- */
typedef struct LrCase {
    int w, h, bd, usize, denom, types[3]; /* w: the upscaled width */
} LrCase;

static void rand_wiener(Rng *r, int16_t *f, int chroma) {
    static const int lo[3] = {-5, -23, -17}, hi[3] = {10, 8, 46};
    int              t[3];
    for (int k = 0; k < 3; k++) t[k] = lo[k] + (int)rng_below(r, (uint32_t)(hi[k] - lo[k] + 1));
    if (chroma) t[0] = 0;
    f[0] = f[6] = (int16_t)t[0];
    f[1] = f[5] = (int16_t)t[1];
    f[2] = f[4] = (int16_t)t[2];
    f[3]        = (int16_t)(-2 * (t[0] + t[1] + t[2]));
    f[7]        = 0;
}

static int get_px(const Yv12BufferConfig *f, int bd, int p, int y, int x) {
    const int st = f->strides[p > 0];
    return bd > 8 ? CONVERT_TO_SHORTPTR(f->buffers[p])[y * st + x] : f->buffers[p][y * st + x];
}
static void set_px(Yv12BufferConfig *f, int bd, int p, int y, int x, int v) {
    const int st = f->strides[p > 0];
    if (bd > 8)
        CONVERT_TO_SHORTPTR(f->buffers[p])[y * st + x] = (uint16_t)v;
    else
        f->buffers[p][y * st + x] = (uint8_t)v;
}

/* a frame buffer of the upscaled size holding a downscaled picture: crop width fw, coded width fw rounded up to 8;
 * every other sample of the planes is 0 */
static void fill_down(Yv12BufferConfig *f, int bd, int fw, Rng *r, const Yv12BufferConfig *like, int noise) {
    const int maxv = (1 << bd) - 1;
    for (int p = 0; p < 3; p++) {
        const int sx = p > 0, ph = f->crop_heights[sx], pw = f->crop_widths[sx];
        const int crop = (fw + sx) >> sx, coded = ((fw + 7) & ~7) >> sx;
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                int v = 0;
                if (x < crop && like)
                    v = get_px(like, bd, p, y, x) + (int)rng_below(r, 2 * noise + 1) - noise;
                else if (x < crop)
                    v = (x * 3 + y * 2) * (maxv + 1) / 1024 + (int)rng_below(r, (uint32_t)(maxv / 8 + 1)) +
                        ((x / 8 + y / 8) & 1) * (maxv / 16);
                else if (x < coded)
                    v = (int)rng_below(r, (uint32_t)maxv + 1);
                set_px(f, bd, p, y, x, clampi(v, 0, maxv));
            }
    }
}

static void put_planes(GoldenFile *g, const char *tag, int ci, const Yv12BufferConfig *f, int bd, int luma_w) {
    for (int p = 0; p < 3; p++) {
        const int sx = p > 0, pw = luma_w >> sx, ph = f->crop_heights[sx];
        uint16_t *a  = malloc(sizeof(uint16_t) * pw * ph);
        uint8_t  *b  = malloc((size_t)pw * ph);
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) b[y * pw + x] = (uint8_t)(a[y * pw + x] = (uint16_t)get_px(f, bd, p, y, x));
        char nm[64];
        snprintf(nm, sizeof nm, "lr%d_%s%d", ci, tag, p);
        if (bd > 8)
            golden_put2(g, nm, 'H', (uint32_t)ph, (uint32_t)pw, a);
        else
            golden_put2(g, nm, 'B', (uint32_t)ph, (uint32_t)pw, b);
        free(a), free(b);
    }
}

static uint8_t *real_ptr(const Yv12BufferConfig *f, int hb, int p) {
    return hb ? (uint8_t *)CONVERT_TO_SHORTPTR(f->buffers[p]) : f->buffers[p];
}

static void gen_lr(GoldenFile *g) {
    static const LrCase cases[] = {
        {208, 136, 8, 64, 11, {3, 1, 2}},
        {203, 74, 10, 64, 16, {3, 3, 3}}, /* odd upscaled crop width (chroma 102), 102 -> 203 */
        {200, 136, 10, 128, 11, {2, 3, 1}},
    };
    const int ncase = (int)(sizeof(cases) / sizeof(cases[0]));
    Rng       r     = {0x5352000000000002ull};
    int32_t   nc    = ncase;
    golden_put1(g, "nlr", 'i', 1, &nc);
    int32_t *tmpbuf = malloc(RESTORATION_TMPBUF_SIZE);
    for (int ci = 0; ci < ncase; ci++) {
        const LrCase      *c   = &cases[ci];
        const int          hb  = c->bd > 8, fw = scaled(c->w, c->denom);
        Av1Common         *cm  = calloc(1, sizeof(Av1Common));
        PictureControlSet *pcs = calloc(1, sizeof(PictureControlSet));
        cm->child_pcs                         = pcs;
        cm->frm_size.frame_height             = (uint16_t)c->h;
        cm->frm_size.superres_upscaled_height = (uint16_t)c->h;
        set_superres(cm, fw, c->w, c->denom, 1, NULL);
        cm->subsampling_x = cm->subsampling_y = 1;
        cm->use_highbitdepth                  = hb;
        cm->bit_depth                         = c->bd;
        cm->mi_rows                           = ((c->h + 7) & ~7) >> 2;
        int usize[3]                          = {c->usize, c->usize >> 1, c->usize >> 1};
        for (int p = 0; p < 3; p++) pcs->rst_info[p].restoration_unit_size = usize[p];
        svt_av1_alloc_restoration_buffers(pcs, cm);
        /* the deblocked and the CDEF picture at the downscaled size, in buffers of the upscaled size */
        Yv12BufferConfig dlf, cdef, up;
        memset(&dlf, 0, sizeof dlf);
        memset(&cdef, 0, sizeof cdef);
        memset(&up, 0, sizeof up);
        svt_aom_realloc_frame_buffer(&dlf, c->w, c->h, 1, 1, hb, 32, 0, NULL, NULL, NULL);
        svt_aom_realloc_frame_buffer(&cdef, c->w, c->h, 1, 1, hb, 32, 0, NULL, NULL, NULL);
        svt_aom_realloc_frame_buffer(&up, c->w, c->h, 1, 1, hb, 32, 0, NULL, NULL, NULL);
        fill_down(&dlf, c->bd, fw, &r, NULL, 0);
        fill_down(&cdef, c->bd, fw, &r, &dlf, 3 << (c->bd - 8));
        put_planes(g, "dlf", ci, &dlf, c->bd, (fw + 7) & ~7);
        put_planes(g, "cdef", ci, &cdef, c->bd, (fw + 7) & ~7);
        /* EbCdefProcess.c:664-677: the boundary lines (the deblocked ones upscaled row pair by row pair), then the
         * upscale of the CDEF frame */
        svt_av1_loop_restoration_save_boundary_lines(&dlf, cm, 0);
        svt_av1_loop_restoration_save_boundary_lines(&cdef, cm, 1);
        for (int p = 0; p < 3; p++) {
            const int s = p > 0;
            svt_av1_upscale_normative_rows(cm, real_ptr(&cdef, hb, p), cdef.strides[s], real_ptr(&up, hb, p),
                                           up.strides[s], (c->h + s) >> s, s, c->bd, hb);
        }
        char    nm[64];
        int32_t prm[7] = {c->w, c->h, c->bd, c->usize, 0, fw, c->denom};
        for (int p = 0; p < 3; p++) {
            RestorationInfo *rsi        = &pcs->rst_info[p];
            rsi->frame_restoration_type = c->types[p] == 0 ? RESTORE_NONE : RESTORE_SWITCHABLE;
            const int nu = rsi->units_per_tile;
            int32_t  *u  = calloc((size_t)nu, 20 * sizeof(int32_t));
            for (int k = 0; k < nu; k++) {
                RestorationUnitInfo *ui = &rsi->unit_info[k];
                memset(ui, 0, sizeof *ui);
                int t = c->types[p] == 3 ? (int)rng_below(&r, 3) : c->types[p];
                if (c->types[p] == 0) t = 0;
                ui->restoration_type = (RestorationType)t;
                rand_wiener(&r, ui->wiener_info.vfilter, p > 0);
                rand_wiener(&r, ui->wiener_info.hfilter, p > 0);
                ui->sgrproj_info.ep     = (int)rng_below(&r, 16);
                ui->sgrproj_info.xqd[0] = -96 + (int)rng_below(&r, 128);
                ui->sgrproj_info.xqd[1] = -32 + (int)rng_below(&r, 128);
                int32_t *e = u + 20 * k;
                e[0]       = t;
                for (int q = 0; q < 8; q++) e[1 + q] = ui->wiener_info.vfilter[q], e[9 + q] = ui->wiener_info.hfilter[q];
                e[17] = ui->sgrproj_info.ep, e[18] = ui->sgrproj_info.xqd[0], e[19] = ui->sgrproj_info.xqd[1];
            }
            snprintf(nm, sizeof nm, "lr%d_units%d", ci, p);
            golden_put2(g, nm, 'i', (uint32_t)nu, 20, u);
            free(u);
            prm[4] |= (c->types[p] != 0) << p;
        }
        snprintf(nm, sizeof nm, "lr%d_params", ci);
        golden_put1(g, nm, 'i', 7, prm);
        svt_av1_loop_restoration_filter_frame(tmpbuf, &up, cm, 0);
        for (int p = 0; p < 3; p++) { /* put_planes takes whole luma widths: the crop width may be odd */
            const int sx = p > 0, pw = up.crop_widths[sx], ph = up.crop_heights[sx];
            uint16_t *a  = malloc(sizeof(uint16_t) * pw * ph);
            uint8_t  *b  = malloc((size_t)pw * ph);
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++)
                    b[y * pw + x] = (uint8_t)(a[y * pw + x] = (uint16_t)get_px(&up, c->bd, p, y, x));
            snprintf(nm, sizeof nm, "lr%d_out%d", ci, p);
            golden_put2(g, nm, hb ? 'H' : 'B', (uint32_t)ph, (uint32_t)pw, hb ? (void *)a : (void *)b);
            free(a), free(b);
        }
        free(dlf.buffer_alloc);
        free(cdef.buffer_alloc);
        free(up.buffer_alloc);
    }
    free(tmpbuf);
}

/* scripts/superres_perf.py's workload (2560 -> 3840 x 2160, 10-bit, three planes) through the reference's C */
static void time_reference(void) {
    const int  fw = 2560, uw = 3840, h = 2160;
    Av1Common *cm = calloc(1, sizeof(Av1Common));
    set_superres(cm, fw, uw, 12, 1, NULL);
    double best = 1e30;
    Rng    r    = {0x5352000000000003ull};
    uint16_t *src[3], *dst[3];
    for (int p = 0; p < 3; p++) {
        const int s = p > 0, ss = (fw >> s) + 2 * BORDER, rows = h >> s;
        src[p] = malloc(sizeof(uint16_t) * ss * rows);
        dst[p] = malloc(sizeof(uint16_t) * (uw >> s) * rows);
        for (int i = 0; i < ss * rows; i++) src[p][i] = (uint16_t)rng_below(&r, 1024);
    }
    uint64_t sum = 0;
    for (int rep = 0; rep < 3; rep++) {
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int p = 0; p < 3; p++) {
            const int s = p > 0;
            svt_av1_upscale_normative_rows(cm, (uint8_t *)(src[p] + BORDER), (fw >> s) + 2 * BORDER, (uint8_t *)dst[p],
                                           uw >> s, h >> s, s, 10, 1);
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        const double ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
        if (ms < best) best = ms;
    }
    for (int p = 0; p < 3; p++)
        for (int i = 0; i < (uw >> (p > 0)) * (h >> (p > 0)); i += 97) sum += dst[p][i];
    printf("{\"workload\": \"2560->3840 x 2160 10-bit, three planes\", \"reference_c_ms\": %.2f, \"reps\": 3, "
           "\"sample_sum\": %llu}\n", best, (unsigned long long)sum);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    bind_c_kernels();
    if (!strcmp(argv[1], "--time")) {
        time_reference();
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    gen_scaled(&g);
    gen_upscale(&g);
    gen_lr(&g);
    golden_close(&g);
    return 0;
}
