/*
 * gen_golden_interp.c — writes tests/golden/interp.bin: the reference's single-reference interpolation family
 * (svt_av1_convolve_{2d,x,y,2d_copy}_sr_c and svt_av1_highbd_convolve_*_sr_c, EbInterPrediction.c:320-427, :679-786), its six
 * filter tables, and the temporal filter's motion compensation (tf_64x64_inter_prediction / tf_32x32_inter_prediction,
 * EbTemporalFiltering.c:2230-2580, through the reference's own svt_aom_inter_prediction) on deterministic inputs, plus one
 * predict -> filter chain per bit depth (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration) and the reference's AVX2 / SSSE3 convolve sources, compiled straight from its tree.
 * EbTemporalFiltering.c is included below, not linked: the two prediction functions and apply_filtering_block_plane_wise
 * are static there, and the generator calls those functions themselves on a minimal scs / pcs / MeContext.  Run from
 * the repository root (REF = the reference checkout; the binary and the objects go outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/interp_simd
 *   for f in ASM_AVX2/convolve_avx2 ASM_AVX2/convolve_2d_avx2 ASM_AVX2/highbd_convolve_avx2 \
 *       ASM_AVX2/highbd_convolve_2d_avx2 ASM_SSSE3/highbd_convolve_ssse3 ASM_SSSE3/highbd_convolve_2d_ssse3 \
 *       ASM_SSE2/EbPictureOperators_Intrinsic_SSE2; do
 *     gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 \
 *       -I$C/ASM_SSSE3 -I$C/ASM_SSE4_1 -c $C/$f.c -o /tmp/interp_simd/$(basename $f).o; done
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_interp.c \
 *     /tmp/interp_simd/*.o -o /tmp/gen_golden_interp -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc \
 *     -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_interp tests/golden/interp.bin
 *   /tmp/gen_golden_interp --time     # scripts/tf_predict_perf.py's shapes through the reference's C and AVX2, one core
 *
 * (EbPictureOperators_Intrinsic_SSE2.c holds svt_memcpy_intrin_sse, which the SIMD copy functions call.)
 *
 * SIMD: where the CPU has AVX2, every block record is made a second time through the reference's _avx2 function and, at
 * 10 / 12 bits, a third time through its _ssse3 function, and must be equal or the generator stops; every prediction
 * record is made a second time with the eight RTCD pointers bound to the _avx2 functions (svt_aom_convolve[][][] /
 * svt_aom_convolveHbd[][][] rebuilt from them) and must be equal.  The 8-bit functions have no SSSE3 form in the
 * reference (their other forms are SSE2 and AVX-512, not compared here).  The file regenerates byte-identically.
 *
 * Inputs that tests/interp_cases.py rebuilds instead of reading are "drawn": sample i of stream `seed` is
 * SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) % mod, golden_io.h's generator started at seed + i * the constant.
 *
 * Records (golden_io format):
 *   tables    h[6][16][8]   sub_pel_filters_8, _8smooth, _8sharp, bilinear_filters, sub_pel_filters_4, _4smooth as compiled
 *   nblock, b<i>_par i32[9] {bd, w, h, phase_x, phase_y, kind, content, form, i}, b<i>_out [h][w], b<i>_mm i32[2] {min, max}
 *             kind 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR for both directions, the parameters
 *             through av1_get_convolve_filter_params (w <= 4 / h <= 4 take the 4-tap tables); form 0 copy, 1 x, 2 y, 3 2d: the
 *             function, chosen by the phases being non-zero as svt_inter_predictor does; rounds from
 *             get_conv_params_no_round.  The source is a drawn (h + 8) x (w + 8) buffer (seed 0x4950000000000000 + 16 * i)
 *             with the block at (3, 3): content 0 noise, 1 all zero, 2 all max, 3 max / zero checkerboard ((x + y) & 1).
 *   npred, p<i>_par i32[7] {bd, w, h, n_refs, tf_chroma, border, i}, p<i>_use64 B[n_refs][nblk], _mv64 h[..][2], _split32
 *             B[..][4], _split16 B[..][16], _mv32 h[..][4][2], _mv16 h[..][16][2], _mv8 h[..][64][2] ((x, y); indices as
 *             MeContext's), p<i>_pred<r>_<p> [ah][aw] the predictor pictures over the 64-aligned area (chroma halved; luma
 *             only when tf_chroma is 0).  Reference picture r, plane p is drawn over the picture (seed 0x4950000000100000 +
 *             256 * i + 4 * r + p, value clamp((2 * x + y) * sc / 4 + draw % (64 * sc))) with edge-replicated borders of
 *             80 luma / 40 chroma samples.
 *   p<i>_kinds i32[12]      how many MVs of the record are: zero, integer, of luma phase 2 / 6 / 10 / 14 in x or y (4 counts),
 *             changed by the clamp at the left / right / top / bottom, wholly outside the picture after it, of odd chroma phase.
 *             The generator stops unless every count of every record is non-zero.
 *   nchain, c<i>_par i32[4] {pred record, mv_dist_th, tf_chroma, i}, c<i>_decay u32[3], c<i>_err32 u64[n_refs][nblk][4],
 *             c<i>_err16 u64[..][16], c<i>_out<p> [h][w]: the predictors of that record fed to the block walk of
 *             produce_temporally_filtered_pic (:2939-3301, as gen_golden_tf.c walks it); the centre is drawn (seed
 *             0x4950000000200000 + 16 * i + p, the same formula); split / mv32 / mv16 are the prediction record's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbTemporalFiltering.c"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "golden_io.h"

void svt_aom_asm_set_convolve_asm_table(void);
void svt_aom_asm_set_convolve_hbd_asm_table(void);
/* the reference's SIMD forms (common_dsp_rtcd.h declares them only under ARCH_X86_64, which the C-only library's headers
 * are not compiled with): AomConvolveFn / aom_highbd_convolve_fn_t */
#define SIMD_8(n) \
    void n(const uint8_t *, int32_t, uint8_t *, int32_t, int32_t, int32_t, InterpFilterParams *, InterpFilterParams *, \
           const int32_t, const int32_t, ConvolveParams *)
#define SIMD_16(n)                                                                                              \
    void n(const uint16_t *, int32_t, uint16_t *, int32_t, int32_t, int32_t, const InterpFilterParams *, \
           const InterpFilterParams *, const int32_t, const int32_t, ConvolveParams *, int32_t)
SIMD_8(svt_av1_convolve_2d_copy_sr_avx2);
SIMD_8(svt_av1_convolve_x_sr_avx2);
SIMD_8(svt_av1_convolve_y_sr_avx2);
SIMD_8(svt_av1_convolve_2d_sr_avx2);
SIMD_16(svt_av1_highbd_convolve_2d_copy_sr_avx2);
SIMD_16(svt_av1_highbd_convolve_x_sr_avx2);
SIMD_16(svt_av1_highbd_convolve_y_sr_avx2);
SIMD_16(svt_av1_highbd_convolve_2d_sr_avx2);
SIMD_16(svt_av1_highbd_convolve_2d_copy_sr_ssse3);
SIMD_16(svt_av1_highbd_convolve_x_sr_ssse3);
SIMD_16(svt_av1_highbd_convolve_y_sr_ssse3);
SIMD_16(svt_av1_highbd_convolve_2d_sr_ssse3);
/* form 0 copy, 1 x, 2 y, 3 2d; pass 0 the _c functions, 1 _avx2, 2 _ssse3 (highbd only) */
static const AomConvolveFn g_fn8[2][4] = {
    {svt_av1_convolve_2d_copy_sr_c, svt_av1_convolve_x_sr_c, svt_av1_convolve_y_sr_c, svt_av1_convolve_2d_sr_c},
    {svt_av1_convolve_2d_copy_sr_avx2, svt_av1_convolve_x_sr_avx2, svt_av1_convolve_y_sr_avx2, svt_av1_convolve_2d_sr_avx2}};
static const aom_highbd_convolve_fn_t g_fn16[3][4] = {
    {svt_av1_highbd_convolve_2d_copy_sr_c, svt_av1_highbd_convolve_x_sr_c, svt_av1_highbd_convolve_y_sr_c,
     svt_av1_highbd_convolve_2d_sr_c},
    {svt_av1_highbd_convolve_2d_copy_sr_avx2, svt_av1_highbd_convolve_x_sr_avx2, svt_av1_highbd_convolve_y_sr_avx2,
     svt_av1_highbd_convolve_2d_sr_avx2},
    {svt_av1_highbd_convolve_2d_copy_sr_ssse3, svt_av1_highbd_convolve_x_sr_ssse3, svt_av1_highbd_convolve_y_sr_ssse3,
     svt_av1_highbd_convolve_2d_sr_ssse3}};
/* the eight RTCD pointers and the two tables the inter predictors call, on the _c (0) or the _avx2 (1) functions */
static void bind_convolve(int pass) {
    svt_av1_convolve_2d_copy_sr = g_fn8[pass][0], svt_av1_convolve_x_sr = g_fn8[pass][1];
    svt_av1_convolve_y_sr = g_fn8[pass][2], svt_av1_convolve_2d_sr = g_fn8[pass][3];
    svt_av1_highbd_convolve_2d_copy_sr = g_fn16[pass][0], svt_av1_highbd_convolve_x_sr = g_fn16[pass][1];
    svt_av1_highbd_convolve_y_sr = g_fn16[pass][2], svt_av1_highbd_convolve_2d_sr = g_fn16[pass][3];
    svt_aom_asm_set_convolve_asm_table();
    svt_aom_asm_set_convolve_hbd_asm_table();
}

static int g_simd; /* the CPU has AVX2: the SIMD passes run */

static uint32_t draw(uint64_t seed, uint64_t i, uint32_t mod) {
    Rng r = {seed + i * 0x9E3779B97F4A7C15ull};
    return (uint32_t)(rng_next(&r) % mod);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

static GoldenFile *g_file;
static const char *nm(const char *fmt, int i, int a, int b) {
    static char s[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(s[k], sizeof s[k], fmt, i, a, b);
    return s[k];
}
static void put(const char *name, char dt, int ndim, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, const void *data) {
    uint32_t dims[4] = {d0, d1, d2, d3};
    golden_put(g_file, name, dt, ndim, dims, data);
}
/* a plane of 16-bit working samples as u8 / u16 */
static void put_plane(const char *name, int bd, int h, int w, const uint16_t *a, int stride) {
    uint16_t *t  = malloc(sizeof(uint16_t) * w * h);
    uint8_t  *t8 = malloc((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) t[y * w + x] = a[y * stride + x], t8[y * w + x] = (uint8_t)a[y * stride + x];
    put(name, bd > 8 ? 'H' : 'B', 2, h, w, 0, 0, bd > 8 ? (void *)t : (void *)t8);
    free(t), free(t8);
}

/* ---- tables ---- */
static void gen_tables(void) {
    int16_t t[6][16][8];
    memcpy(t[0], sub_pel_filters_8, sizeof t[0]), memcpy(t[1], sub_pel_filters_8smooth, sizeof t[0]);
    memcpy(t[2], sub_pel_filters_8sharp, sizeof t[0]), memcpy(t[3], bilinear_filters, sizeof t[0]);
    memcpy(t[4], sub_pel_filters_4, sizeof t[0]), memcpy(t[5], sub_pel_filters_4smooth, sizeof t[0]);
    put("tables", 'h', 3, 6, 16, 8, 0, t);
}

/* ---- block records ---- */
static void fill_block(uint16_t *s, int bd, int w, int h, int content, uint64_t seed) {
    const int maxv = (1 << bd) - 1, bw = w + 8, bh = h + 8;
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++)
            s[y * bw + x] = (uint16_t)(content == 0 ? draw(seed, (uint64_t)y * bw + x, maxv + 1)
                                                    : content == 1 ? 0 : content == 2 ? maxv : ((x + y) & 1) ? maxv : 0);
}
static void run_block(int pass, int bd, int w, int h, int phx, int phy, int kind, const uint16_t *s, uint16_t *out) {
    const int          bw = w + 8, form = (phx ? 1 : 0) | (phy ? 2 : 0);
    InterpFilterParams px, py;
    ConvolveParams     cp = get_conv_params_no_round(0, 0, 0, NULL, 0, 0, bd);
    av1_get_convolve_filter_params(av1_make_interp_filters((InterpFilter)kind, (InterpFilter)kind), &px, &py, w, h);
    if (bd == 8) {
        uint8_t *s8 = malloc((size_t)bw * (h + 8)), *o8 = malloc((size_t)w * h);
        for (int i = 0; i < bw * (h + 8); i++) s8[i] = (uint8_t)s[i];
        g_fn8[pass][form](s8 + 3 * bw + 3, bw, o8, w, w, h, &px, &py, phx, phy, &cp);
        for (int i = 0; i < w * h; i++) out[i] = o8[i];
        free(s8), free(o8);
    } else {
        g_fn16[pass][form](s + 3 * bw + 3, bw, out, w, w, h, &px, &py, phx, phy, &cp, bd);
    }
}
static int gen_blocks(void) {
    static const int sizes[12][2] = {{2, 2}, {2, 4}, {4, 4}, {4, 16}, {16, 4}, {8, 8}, {8, 32}, {16, 16}, {32, 32}, {64, 16},
                                     {64, 64}, {128, 128}};
    static const int ph[4] = {0, 1, 8, 15}, bds[3] = {8, 10, 12};
    int              n = 0, seen[2][4] = {{0}}, lo[2][4] = {{0}}, hi[2][4] = {{0}};
    uint16_t        *s = malloc(sizeof(uint16_t) * 136 * 136), *o = malloc(sizeof(uint16_t) * 128 * 128);
    uint16_t        *o2 = malloc(sizeof(uint16_t) * 128 * 128);
    for (int si = 0; si < 12; si++)
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                const int w = sizes[si][0], h = sizes[si][1];
                /* the two largest sizes: one record per form; every other size: all sixteen phase pairs */
                if (w * h >= 4096 && !((a == 0 || a == 2) && (b == 0 || b == 3))) continue;
                /* bit depth and kind rotate with the record; the content with the records of one function (zero, max,
                 * checkerboard, noise in turn), so that every function meets each content */
                const int phx = ph[a], phy = ph[b], form = (phx ? 1 : 0) | (phy ? 2 : 0);
                const int bd = bds[n % 3], kind = (n / 3) & 3, content = (1 + seen[bd > 8][form]) & 3;
                fill_block(s, bd, w, h, content, 0x4950000000000000ull + 16 * (uint64_t)n);
                run_block(0, bd, w, h, phx, phy, kind, s, o);
                for (int pass = 1; g_simd && pass <= (bd > 8 ? 2 : 1); pass++) {
                    memset(o2, 0xA5, sizeof(uint16_t) * w * h);
                    run_block(pass, bd, w, h, phx, phy, kind, s, o2);
                    if (memcmp(o, o2, sizeof(uint16_t) * w * h))
                        fprintf(stderr, "%s != c: block record %d (%dx%d, %d bits, form %d)\n", pass == 1 ? "avx2" : "ssse3", n, w, h, bd, form), exit(3);
                }
                int32_t mm[2] = {65535, 0}, par[9] = {bd, w, h, phx, phy, kind, content, form, n};
                for (int i = 0; i < w * h; i++) mm[0] = o[i] < mm[0] ? o[i] : mm[0], mm[1] = o[i] > mm[1] ? o[i] : mm[1];
                put(nm("b%d_par", n, 0, 0), 'i', 1, 9, 0, 0, 0, par);
                put_plane(nm("b%d_out", n, 0, 0), bd, h, w, o, w);
                put(nm("b%d_mm", n, 0, 0), 'i', 1, 2, 0, 0, 0, mm);
                seen[bd > 8][form]++, lo[bd > 8][form] |= mm[0] == 0, hi[bd > 8][form] |= mm[1] == (1 << bd) - 1;
                n++;
            }
    for (int k = 0; k < 8; k++)
        if (!seen[k >> 2][k & 3] || !lo[k >> 2][k & 3] || !hi[k >> 2][k & 3])
            fprintf(stderr, "function %d: not hit, or a clip end not reached\n", k), exit(3);
    int32_t nn = n;
    put("nblock", 'i', 1, 1, 0, 0, 0, &nn);
    free(s), free(o), free(o2);
    return n;
}

/* ---- prediction records ---- */
#define PAD 80
typedef struct Motion {
    uint8_t use64, split32[4], split16[16];
    int16_t mv64[2], mv32[4][2], mv16[16][2], mv8[64][2];
} Motion;
typedef struct RefPic { /* one padded reference picture, as 16-bit and as 8-bit samples */
    uint16_t *p16[3];
    uint8_t  *p8[3];
    int       stride[3];
} RefPic;
typedef struct PredPic { /* the 64-aligned area, 16-bit working samples */
    uint16_t *p[3];
    int       aw, ah;
} PredPic;

static int pic_value(int bd, uint64_t seed, int pw, int x, int y) {
    const int sc = 1 << (bd - 8);
    return clampi((2 * x + y) * sc / 4 + (int)draw(seed, (uint64_t)y * pw + x, 64 * sc), 0, (1 << bd) - 1);
}
static void ref_alloc(RefPic *r, int bd, int w, int h, uint64_t seed) {
    for (int p = 0; p < 3; p++) {
        const int ss = p > 0, pw = w >> ss, ph = h >> ss, pad = PAD >> ss, st = pw + 2 * pad;
        r->stride[p] = st;
        r->p16[p] = malloc(sizeof(uint16_t) * st * (ph + 2 * pad)), r->p8[p] = malloc((size_t)st * (ph + 2 * pad));
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) r->p16[p][(y + pad) * st + x + pad] = (uint16_t)pic_value(bd, seed + p, pw, x, y);
        for (int y = -pad; y < ph + pad; y++)
            for (int x = -pad; x < pw + pad; x++) {
                const uint16_t v = r->p16[p][(clampi(y, 0, ph - 1) + pad) * st + clampi(x, 0, pw - 1) + pad];
                r->p16[p][(y + pad) * st + x + pad] = v, r->p8[p][(y + pad) * st + x + pad] = (uint8_t)v;
            }
    }
}
static void ref_free(RefPic *r) {
    for (int p = 0; p < 3; p++) free(r->p16[p]), free(r->p8[p]);
}

static int16_t draw_mv(Rng *r, int w) {
    switch (rng_below(r, 8)) {
    case 0: return 0;
    case 1: return (int16_t)(8 * ((int)rng_below(r, 33) - 16));
    case 5: return (int16_t)((int)rng_below(r, 4001) - 2000);
    case 6: return (int16_t)((rng_below(r, 2) ? 1 : -1) * (w * 8 + 1000 + (int)rng_below(r, 64)));
    case 7: return (int16_t)(2 * ((int)rng_below(r, 9) - 4) + 1);
    default: return (int16_t)((int)rng_below(r, 129) - 64);
    }
}
static void draw_motion(Motion *m, int n, Rng *r, int w) {
    for (int k = 0; k < n; k++, m++) {
        m->use64 = (uint8_t)(k == 0 || (k > 1 && !rng_below(r, 4)));
        for (int i = 0; i < 4; i++) m->split32[i] = (uint8_t)(k == 1 ? (i == 1 || i == 2) : rng_below(r, 2));
        for (int i = 0; i < 16; i++) m->split16[i] = (uint8_t)(k == 1 ? (i & 1) : rng_below(r, 2));
        m->mv64[0] = draw_mv(r, w), m->mv64[1] = draw_mv(r, w);
        for (int i = 0; i < 4; i++) m->mv32[i][0] = draw_mv(r, w), m->mv32[i][1] = draw_mv(r, w);
        for (int i = 0; i < 16; i++) m->mv16[i][0] = draw_mv(r, w), m->mv16[i][1] = draw_mv(r, w);
        for (int i = 0; i < 64; i++) m->mv8[i][0] = draw_mv(r, w), m->mv8[i][1] = draw_mv(r, w);
    }
}
static void motion_to_ctx(const Motion *m, MeContext *c) {
    c->tf_64x64_mv_x = m->mv64[0], c->tf_64x64_mv_y = m->mv64[1];
    for (int i = 0; i < 4; i++) {
        c->tf_32x32_block_split_flag[i] = m->split32[i];
        c->tf_32x32_mv_x[i] = m->mv32[i][0], c->tf_32x32_mv_y[i] = m->mv32[i][1];
    }
    for (int i = 0; i < 16; i++) {
        c->tf_16x16_block_split_flag[i >> 2][i & 3] = m->split16[i];
        c->tf_16x16_mv_x[i] = m->mv16[i][0], c->tf_16x16_mv_y[i] = m->mv16[i][1];
    }
    for (int i = 0; i < 64; i++) c->tf_8x8_mv_x[i] = m->mv8[i][0], c->tf_8x8_mv_y[i] = m->mv8[i][1];
}
/* the kinds of one MV that the compensation uses: block of size b at (px, py), luma arithmetic restated for the count only */
static void count_mv(int32_t kinds[12], int mvx, int mvy, int px, int py, int b, int w, int h) {
    const int mv[2] = {mvx, mvy}, org[2] = {px, py}, dim[2] = {w, h};
    kinds[0] += !mvx && !mvy;
    kinds[1] += (mvx || mvy) && !(mvx & 7) && !(mvy & 7);
    for (int d = 0; d < 2; d++) {
        const int q = (int16_t)(mv[d] * 2), lo = -org[d] * 16 - ((4 + b) << 4), hi = (dim[d] - b - org[d]) * 16 + ((4 + b) << 4) - 16;
        const int c = clampi(q, lo, hi), pos = org[d] + (c >> 4);
        for (int k = 0; k < 4; k++) kinds[2 + k] += (c & 15) == 2 + 4 * k;
        kinds[6 + 2 * d] += q < lo, kinds[7 + 2 * d] += q > hi;
        kinds[10] += pos + b <= 0 || pos >= dim[d];
        kinds[11] += (mv[d] & 1);
    }
}

static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_pcs, *g_pcs_ref;
static void                     setup_reference(int w, int h) {
    if (!g_scs) {
        svt_aom_setup_common_rtcd_internal(0);
        svt_aom_setup_rtcd_internal(0);
        svt_aom_asm_set_convolve_asm_table();
        svt_aom_asm_set_convolve_hbd_asm_table();
        svt_aom_build_blk_geom(GEOM_0);
        g_scs = calloc(1, sizeof *g_scs), g_pcs = calloc(1, sizeof *g_pcs), g_pcs_ref = calloc(1, sizeof *g_pcs_ref);
        g_pcs->scs = g_scs, g_pcs->av1_cm = calloc(1, sizeof(Av1Common));
        g_scs->seq_header.sb_size = BLOCK_64X64;
    }
    svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, w, h, w, h);
    g_pcs->av1_cm->mi_rows = h / 4, g_pcs->av1_cm->mi_cols = w / 4;
}

/* the predictor picture of one reference: per 64x64 block tf_64x64_inter_prediction or the four tf_32x32_inter_prediction
 * calls, exactly as produce_temporally_filtered_pic makes them (:3087-3260), copied into the picture */
static void predict_picture(int bd, int w, int h, int chroma, RefPic *ref, const Motion *motion, PredPic *out, int32_t *kinds) {
    DECLARE_ALIGNED(32, uint16_t, pr16[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint8_t, pr8[BLK_PELS * COLOR_CHANNELS]);
    uint16_t           *pred16[3] = {pr16, pr16 + BLK_PELS, pr16 + 2 * BLK_PELS};
    uint8_t            *pred8[3]  = {pr8, pr8 + BLK_PELS, pr8 + 2 * BLK_PELS};
    MeContext          *ctx = calloc(1, sizeof *ctx);
    EbPictureBufferDesc desc;
    memset(&desc, 0, sizeof desc);
    desc.buffer_y = ref->p8[0], desc.buffer_cb = ref->p8[1], desc.buffer_cr = ref->p8[2];
    desc.org_x = PAD, desc.org_y = PAD, desc.width = (uint16_t)w, desc.height = (uint16_t)h;
    desc.stride_y = (uint16_t)ref->stride[0], desc.stride_cb = (uint16_t)ref->stride[1], desc.stride_cr = (uint16_t)ref->stride[2];
    for (int p = 0; p < 3; p++) g_pcs_ref->altref_buffer_highbd[p] = ref->p16[p];
    ctx->tf_chroma     = (uint8_t)chroma;
    const int blk_cols = (w + 63) / 64, blk_rows = (h + 63) / 64;
    for (int br = 0; br < blk_rows; br++)
        for (int bc = 0; bc < blk_cols; bc++) {
            const Motion *m = &motion[br * blk_cols + bc];
            motion_to_ctx(m, ctx);
            memset(pr16, 0, sizeof pr16), memset(pr8, 0, sizeof pr8);
            if (m->use64) {
                tf_64x64_inter_prediction(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, bc * 64, br * 64, 1, bd);
                if (kinds) count_mv(kinds, m->mv64[0], m->mv64[1], bc * 64, br * 64, 64, w, h);
            } else
                for (int i = 0; i < 4; i++) {
                    ctx->idx_32x32 = i;
                    tf_32x32_inter_prediction(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, bc * 64, br * 64, 1, bd);
                    const int x32 = bc * 64 + (i & 1) * 32, y32 = br * 64 + (i >> 1) * 32;
                    if (!kinds) continue;
                    if (!m->split32[i]) count_mv(kinds, m->mv32[i][0], m->mv32[i][1], x32, y32, 32, w, h);
                    for (int j = 0; m->split32[i] && j < 4; j++) {
                        const int x16 = x32 + (j & 1) * 16, y16 = y32 + (j >> 1) * 16, q = 4 * i + j;
                        if (!m->split16[q]) count_mv(kinds, m->mv16[q][0], m->mv16[q][1], x16, y16, 16, w, h);
                        for (int k = 0; m->split16[q] && k < 4; k++)
                            count_mv(kinds, m->mv8[4 * q + k][0], m->mv8[4 * q + k][1], x16 + (k & 1) * 8, y16 + (k >> 1) * 8, 8, w, h);
                    }
                }
            for (int p = 0; p < (chroma ? 3 : 1); p++) {
                const int ss = p > 0, bw = 64 >> ss, aw = out->aw >> ss;
                for (int y = 0; y < bw; y++)
                    for (int x = 0; x < bw; x++)
                        out->p[p][((br * 64 >> ss) + y) * aw + (bc * 64 >> ss) + x] = bd > 8 ? pred16[p][y * bw + x] : pred8[p][y * bw + x];
            }
        }
    free(ctx);
}

/* ---- the chain: produce_temporally_filtered_pic's block walk over given predictor pictures (gen_golden_tf.c's) ---- */
static void filter_picture(MeContext *ctx, int bd, int w, int h, PredPic *centre, PredPic *refs, int n_refs, const Motion *motion,
                           const uint64_t *err32, const uint64_t *err16) {
    DECLARE_ALIGNED(32, uint32_t, accumulator[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, counter[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, pr16[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint8_t, pr8[BLK_PELS * COLOR_CHANNELS]);
    uint32_t *accum[3] = {accumulator, accumulator + BLK_PELS, accumulator + 2 * BLK_PELS};
    uint16_t *count[3] = {counter, counter + BLK_PELS, counter + 2 * BLK_PELS};
    uint16_t *pred16[3] = {pr16, pr16 + BLK_PELS, pr16 + 2 * BLK_PELS};
    uint8_t  *pred8[3] = {pr8, pr8 + BLK_PELS, pr8 + 2 * BLK_PELS}, *c8[3];
    uint32_t  stride[3] = {centre->aw, centre->aw / 2, centre->aw / 2}, stride_pred[3] = {BW, BW / 2, BW / 2};
    for (int p = 0; p < 3; p++) {
        const size_t n = (size_t)stride[p] * (centre->ah >> (p > 0));
        c8[p] = malloc(n);
        for (size_t k = 0; k < n; k++) c8[p][k] = (uint8_t)centre->p[p][k];
    }
    EbPictureBufferDesc desc;
    memset(&desc, 0, sizeof desc);
    desc.stride_y      = (uint16_t)stride[0];
    const int blk_cols = (w + BW - 1) / BW, blk_rows = (h + BH - 1) / BH, nblk = blk_cols * blk_rows;
    for (int br = 0; br < blk_rows; br++)
        for (int bc = 0; bc < blk_cols; bc++) {
            const int yoff = bc * BW + br * BH * stride[0], coff = bc * (BW / 2) + br * (BH / 2) * stride[1];
            uint8_t  *s8[3] = {c8[0] + yoff, c8[1] + coff, c8[2] + coff};
            uint16_t *s16[3] = {centre->p[0] + yoff, centre->p[1] + coff, centre->p[2] + coff};
            memset(accumulator, 0, sizeof accumulator), memset(counter, 0, sizeof counter);
            if (bd == 8)
                apply_filtering_central(ctx, &desc, s8, accum, count, BW, BH, 1, 1);
            else
                apply_filtering_central_highbd(ctx, &desc, s16, accum, count, BW, BH, 1, 1);
            for (int r = 0; r < n_refs; r++) {
                for (int p = 0; p < 3; p++) {
                    const int bwp = p ? BW / 2 : BW, off = p ? coff : yoff;
                    for (int y = 0; y < bwp; y++)
                        for (int x = 0; x < bwp; x++) {
                            pred16[p][y * bwp + x] = refs[r].p[p][off + y * stride[p] + x];
                            pred8[p][y * bwp + x]  = (uint8_t)pred16[p][y * bwp + x];
                        }
                }
                const int k = r * nblk + br * blk_cols + bc;
                motion_to_ctx(&motion[k], ctx);
                for (int i = 0; i < 4; i++) ctx->tf_32x32_block_error[i] = err32[4 * k + i];
                for (int i = 0; i < 16; i++) ctx->tf_16x16_block_error[i] = err16[16 * k + i];
                for (int row = 0; row < 2; row++)
                    for (int col = 0; col < 2; col++) {
                        ctx->tf_block_col = col, ctx->tf_block_row = row;
                        apply_filtering_block_plane_wise(ctx, row, col, s8, s16, pred8, pred16, accum, count, stride, stride_pred,
                                                         BW >> 1, BH >> 1, 1, 1, bd);
                    }
            }
            get_final_filtered_pixels(ctx, c8, centre->p, accum, count, stride, yoff, coff, BW / 2, BH / 2, bd > 8);
        }
    for (int p = 0; p < 3; p++) {
        const size_t n = (size_t)stride[p] * (centre->ah >> (p > 0));
        if (bd == 8)
            for (size_t k = 0; k < n; k++) centre->p[p][k] = c8[p][k];
        free(c8[p]);
    }
}

static void pred_alloc(PredPic *p, int w, int h) {
    p->aw = (w + 63) & ~63, p->ah = (h + 63) & ~63;
    for (int k = 0; k < 3; k++) p->p[k] = calloc((size_t)(p->aw >> (k > 0)) * (p->ah >> (k > 0)), sizeof(uint16_t));
}
static void pred_free(PredPic *p) {
    for (int k = 0; k < 3; k++) free(p->p[k]);
}

static void gen_pred(void) {
    static const int cases[4][2] = {{8, 1}, {8, 0}, {10, 1}, {10, 0}}; /* {bd, tf_chroma} */
    const int        w = 136, h = 72, nr = 2, nblk = 6;
    int              nchain = 0;
    setup_reference(w, h);
    for (int i = 0; i < 4; i++) {
        const int bd = cases[i][0], chroma = cases[i][1];
        Rng       r = {0x4950000000080000ull + i};
        Motion   *motion = calloc((size_t)nr * nblk, sizeof(Motion));
        RefPic    refs[2];
        PredPic   pred[2];
        int32_t   kinds[12] = {0}, par[7] = {bd, w, h, nr, chroma, PAD, i};
        draw_motion(motion, nr * nblk, &r, w);
        for (int k = 0; k < nr; k++) {
            ref_alloc(&refs[k], bd, w, h, 0x4950000000100000ull + 256 * (uint64_t)i + 4 * k);
            pred_alloc(&pred[k], w, h);
            predict_picture(bd, w, h, chroma, &refs[k], motion + k * nblk, &pred[k], kinds);
            if (g_simd) { /* the same through svt_aom_inter_prediction on the _avx2 functions */
                PredPic again;
                pred_alloc(&again, w, h);
                bind_convolve(1);
                predict_picture(bd, w, h, chroma, &refs[k], motion + k * nblk, &again, NULL);
                bind_convolve(0);
                for (int p = 0; p < (chroma ? 3 : 1); p++)
                    if (memcmp(again.p[p], pred[k].p[p], sizeof(uint16_t) * (again.aw >> (p > 0)) * (again.ah >> (p > 0))))
                        fprintf(stderr, "avx2 != c: prediction record %d reference %d plane %d\n", i, k, p), exit(3);
                pred_free(&again);
            }
        }
        for (int k = 0; k < 12; k++)
            if (!kinds[k]) fprintf(stderr, "prediction record %d: no MV of kind %d\n", i, k), exit(3);
        put(nm("p%d_par", i, 0, 0), 'i', 1, 7, 0, 0, 0, par);
        put(nm("p%d_kinds", i, 0, 0), 'i', 1, 12, 0, 0, 0, kinds);
        uint8_t *u64 = malloc(nr * nblk), *s32 = malloc(nr * nblk * 4), *s16 = malloc(nr * nblk * 16);
        int16_t *m64 = malloc(nr * nblk * 4), *m32 = malloc(nr * nblk * 16), *m16 = malloc(nr * nblk * 64), *m8 = malloc(nr * nblk * 256);
        for (int k = 0; k < nr * nblk; k++) {
            u64[k] = motion[k].use64, memcpy(s32 + 4 * k, motion[k].split32, 4), memcpy(s16 + 16 * k, motion[k].split16, 16);
            memcpy(m64 + 2 * k, motion[k].mv64, 4), memcpy(m32 + 8 * k, motion[k].mv32, 16);
            memcpy(m16 + 32 * k, motion[k].mv16, 64), memcpy(m8 + 128 * k, motion[k].mv8, 256);
        }
        put(nm("p%d_use64", i, 0, 0), 'B', 2, nr, nblk, 0, 0, u64);
        put(nm("p%d_mv64", i, 0, 0), 'h', 3, nr, nblk, 2, 0, m64);
        put(nm("p%d_split32", i, 0, 0), 'B', 3, nr, nblk, 4, 0, s32);
        put(nm("p%d_split16", i, 0, 0), 'B', 3, nr, nblk, 16, 0, s16);
        put(nm("p%d_mv32", i, 0, 0), 'h', 4, nr, nblk, 4, 2, m32);
        put(nm("p%d_mv16", i, 0, 0), 'h', 4, nr, nblk, 16, 2, m16);
        put(nm("p%d_mv8", i, 0, 0), 'h', 4, nr, nblk, 64, 2, m8);
        free(u64), free(s32), free(s16), free(m64), free(m32), free(m16), free(m8);
        for (int k = 0; k < nr; k++)
            for (int p = 0; p < (chroma ? 3 : 1); p++)
                put_plane(nm("p%d_pred%d_%d", i, k, p), bd, pred[k].ah >> (p > 0), pred[k].aw >> (p > 0), pred[k].p[p], pred[k].aw >> (p > 0));
        if (chroma) { /* the chain record of this bit depth */
            const int  c = nchain++;
            MeContext *ctx = calloc(1, sizeof *ctx);
            PredPic    centre;
            uint64_t  *e32 = malloc(sizeof(uint64_t) * nr * nblk * 4), *e16 = malloc(sizeof(uint64_t) * nr * nblk * 16);
            static const uint32_t decay[3] = {6000000, 9000000, 12000000};
            pred_alloc(&centre, w, h);
            for (int p = 0; p < 3; p++) {
                const int pw = centre.aw >> (p > 0), ph = centre.ah >> (p > 0);
                for (int y = 0; y < ph; y++)
                    for (int x = 0; x < pw; x++)
                        centre.p[p][y * pw + x] = (uint16_t)pic_value(bd, 0x4950000000200000ull + 16 * (uint64_t)c + p, pw, x, y);
            }
            for (int k = 0; k < nr * nblk * 4; k++) e32[k] = (uint64_t)rng_below(&r, 200000) << (bd > 8 ? 4 : 0);
            for (int k = 0; k < nr * nblk * 16; k++) e16[k] = (uint64_t)rng_below(&r, 60000) << (bd > 8 ? 4 : 0);
            memcpy(ctx->tf_decay_factor_fp16, decay, sizeof decay);
            ctx->tf_mv_dist_th = 1080, ctx->tf_chroma = 1;
            filter_picture(ctx, bd, w, h, &centre, pred, nr, motion, e32, e16);
            int32_t cpar[4] = {i, 1080, 1, c};
            put(nm("c%d_par", c, 0, 0), 'i', 1, 4, 0, 0, 0, cpar);
            put(nm("c%d_decay", c, 0, 0), 'I', 1, 3, 0, 0, 0, decay);
            put(nm("c%d_err32", c, 0, 0), 'Q', 3, nr, nblk, 4, 0, e32);
            put(nm("c%d_err16", c, 0, 0), 'Q', 3, nr, nblk, 16, 0, e16);
            for (int p = 0; p < 3; p++) put_plane(nm("c%d_out%d", c, p, 0), bd, h >> (p > 0), w >> (p > 0), centre.p[p], centre.aw >> (p > 0));
            pred_free(&centre), free(e32), free(e16), free(ctx);
        }
        for (int k = 0; k < nr; k++) ref_free(&refs[k]), pred_free(&pred[k]);
        free(motion);
    }
    int32_t np = 4, nc = nchain;
    put("npred", 'i', 1, 1, 0, 0, 0, &np);
    put("nchain", 'i', 1, 1, 0, 0, 0, &nc);
}

/* scripts/tf_predict_perf.py's workloads through the reference's C on one core */
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static void time_reference(void) {
    static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
    for (int k = 0; k < 2; k++) {
        const int bd = shapes[k][0], w = shapes[k][1], h = shapes[k][2], nr = 6, nblk = ((w + 63) / 64) * ((h + 63) / 64);
        Rng       r = {0x4950000000300000ull};
        Motion   *motion = calloc((size_t)nr * nblk, sizeof(Motion));
        RefPic    ref;
        PredPic   pred;
        int       nb[4] = {0, 0, 0, 0}; /* blocks of 64 / 32 / 16 / 8 */
        setup_reference(w, h);
        draw_motion(motion, nr * nblk, &r, w);
        for (int q = 0; q < nr * nblk; q++) {
            const Motion *m = &motion[q];
            nb[0] += m->use64;
            for (int i = 0; !m->use64 && i < 4; i++) {
                nb[1] += !m->split32[i];
                for (int j = 0; m->split32[i] && j < 4; j++) nb[2] += !m->split16[4 * i + j], nb[3] += 4 * m->split16[4 * i + j];
            }
        }
        ref_alloc(&ref, bd, w, h, 0x4950000000400000ull);
        pred_alloc(&pred, w, h);
        double ms[2] = {0, 0};
        for (int pass = 0; pass <= g_simd; pass++) {
            bind_convolve(pass);
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                const double t0 = now_ms();
                for (int q = 0; q < nr; q++) predict_picture(bd, w, h, 1, &ref, motion + q * nblk, &pred, NULL);
                const double t1 = now_ms();
                if (t1 - t0 < best) best = t1 - t0;
            }
            ms[pass] = best;
        }
        bind_convolve(0);
        printf("{\"workload\": \"%dx%d %d-bit, %d references\", \"predict_c_ms\": %.2f, \"predict_avx2_ms\": %.2f, "
               "\"blocks_64_32_16_8\": [%d, %d, %d, %d], \"reps\": 3}\n", w, h, bd, nr, ms[0], ms[1], nb[0], nb[1], nb[2], nb[3]);
        ref_free(&ref), pred_free(&pred), free(motion);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    g_simd = __builtin_cpu_supports("avx2") ? 1 : 0;
    if (!strcmp(argv[1], "--time")) {
        time_reference();
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    gen_tables();
    const int nb = gen_blocks();
    gen_pred();
    golden_close(&g);
    fprintf(stderr, "%d block records, 4 prediction records, 2 chain records; %s\n", nb,
            g_simd ? "every block record equal through the _avx2 (and at 10 / 12 bits the _ssse3) functions, every prediction "
                     "record equal through the _avx2 functions"
                   : "no AVX2 on this host: the _c functions only");
    return 0;
}
