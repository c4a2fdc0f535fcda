/*
 * gen_golden_warp.c — writes tests/golden/warp.bin: the reference's warped-motion prediction: the warped filter table and
 * the divisor table of resolve_divisor_32, svt_get_shear_params (EbWarpedMotion.c:1082-1105), svt_av1_warp_affine_c /
 * svt_av1_highbd_warp_affine_c (:570, :822) and svt_aom_warped_motion_prediction (EbEncInterPrediction.c:2747) on
 * deterministic inputs (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration) and the reference's AVX2 sources of the two functions, compiled straight from its tree.  Run from the
 * repository root (REF = the reference checkout; the binary and the objects go outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/warp_simd
 *   for f in ASM_AVX2/warp_plane_avx2 ASM_AVX2/highbd_warp_affine_avx2; do
 *     gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 \
 *       -I$C/ASM_SSSE3 -I$C/ASM_SSE4_1 -c $C/$f.c -o /tmp/warp_simd/$(basename $f).o; done
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_warp.c \
 *     /tmp/warp_simd/*.o -o /tmp/gen_golden_warp -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc \
 *     -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_warp tests/golden/warp.bin
 *   /tmp/gen_golden_warp --time   # scripts/warp_perf.py's lists through the reference's C, one core (profiles/warp/reference_time.log)
 *
 * SIMD: both AVX2 forms compile stand-alone.  Where the CPU has AVX2, every unit record is made a second time through the
 * reference's _avx2 function and every batch record a second time with the two RTCD pointers bound to the _avx2 functions;
 * the generator stops on a difference.  (The AVX2 forms have paths of their own for ix4 <= -7 and ix4 >= width + 6; the
 * models that put the origin outside the plane take them.)  Without the two objects on the link line the generator builds
 * and runs on the C alone (the _avx2 symbols are weak).  The file regenerates byte-identically.
 *
 * Drawn inputs: sample i of stream `seed` is SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) % mod, as in
 * gen_golden_compound.c.
 *
 * Records (golden_io format):
 *   filter h[193][8]     svt_aom_warped_filter.
 *   div_lut i[257]       the divisor table, static in the reference and so read through svt_get_shear_params: with wmmat[2] =
 *                        256 + f (and 1023 for f = 256) and wmmat[3] * wmmat[4] = 2^22 (2^23 there), delta is wmmat[5] - 65536 -
 *                        div_lut[f] reduced to a multiple of 64 with signed rounding, which is 0 from wmmat[5] - 65536 =
 *                        div_lut[f] - 31 on and -64 below.
 *   shear_in i[n][6], shear_out i[n][5] {return value, alpha, beta, gamma, delta as the reference leaves them in the model
 *                        (all zero going in)}; shear_kinds i[12]: models with wmmat[2] <= 0, pure translations, just allowed /
 *                        just refused at the first limit, the same at the second, -32768 in alpha / beta / gamma / delta (a
 *                        clamp at either end: 32767 rounds to 32768 and wraps), negative deviations accepted, the count.
 *   nunit, u<i>_par i[16] {bd, plane width, plane height, p_col, p_row, p_width, p_height, ss, mode (0 not compound, 1
 *                        compound average, 2 compound distance-weighted), content, model, second model, fwd_offset, bck_offset,
 *                        i, flip}, u<i>_mat i[2][6], u<i>_abgd i[2][4].  The reference plane of pass s (0 first, 1 second) has sample
 *                        (x, y) = content 0: draw(0x5750000000000000 + 16 * i + 8 * s, y * width + x, max + 1), max = 2^min(bd, 10) - 1 (the
 *                        split layout holds ten bits at any bd); 1: 0; 2: max; 3: max
 *                        where tap x % 8 of filter row 96 (the half-sample row) is positive, else 0, inverted when s != flip; 4: the
 *                        same by y % 8.  u<i>_out [p_height][p_width] the pixels (mode 0: of pass 0 with model 0; else of pass 1 with the
 *                        second model on u<i>_conv); u<i>_conv H[p_height][p_width] the first pass's CONV_BUF_TYPE block (modes
 *                        1, 2).  8 bits through svt_av1_warp_affine_c, 10 and 12 through svt_av1_highbd_warp_affine_c on the
 *                        split planes (v >> 2, (v & 3) << 6).  unit_kinds i[16]: horizontal filter row 0 reached, row 192, vertical
 *                        filter row 0, row 176 (its last: 8 rows, not 15), an output of 0, of max, a compound record per pattern
 *                        content (2), units with ix4 <= -7, ix4 >= width + 6 (the AVX2 forms' own paths), iy4 <= -7, iy4 >= height
 *                        + 6 (4), units further out than the plane is wide or high on each side (4).  unit_tmp i[3][4] per bit depth
 *                        8, 10, 12 {min, max of the horizontal intermediate over all records (the C's tmp[], restated in the
 *                        generator), the smallest sum of negative taps and the largest of positive taps of a table row}: the
 *                        generator stops unless min and max are the analytic ends (offset + that sum * max, rounded), which the
 *                        last fifteen records reach (a pure translation onto the table's heaviest row, 93, over the pattern
 *                        contents), unless the maximum fits 16 bits, and unless the outputs reach both clips (12 bits: the
 *                        lower one; ten-bit samples cannot reach 4095).
 *   nbatch, q<i>_par i[8] {bd, w, h, n_refs, chroma, n_blocks, i, 0}, q<i>_blocks i[n_blocks][22] {x, y, w, h, ref0, ref1 (255:
 *                        one reference), dist_wtd, fwd_offset, bck_offset, 0, wmmat0[6], wmmat1[6]}, q<i>_pred<p> the predictor
 *                        planes, zero where nothing was written (luma only when chroma is 0; blocks below 16 in a dimension
 *                        are predicted with the luma mask: their chroma is a translation in the reference and no part of the
 *                        fixture).  Reference pictures: plane p of reference r has sample (x, y) = clamp((2x + y) * 2^(bd - 8)
 *                        / 4 + draw(0x5750000000100000 + 256 * i + 4 * r + p, y * pw + x, 64 * 2^(bd - 8))), no border.
 *   q<i>_kinds i[24]     blocks of 8x8, h = 4w, w = 4h, 16x16, at least 64x64 (5); a one-reference block next to a
 *                        two-reference one; average; distance-weighted; ref0 == ref1 with equal models; at each picture corner
 *                        (4); below 16 in a dimension; with a luma unit clamped at the left, right, top, bottom (4); with a
 *                        negative dst_x, dst_y (2); one-reference blocks; the count; 128x64 blocks (zero in the first record, whose
 *                        tiling has a 64x64 and a 16x64 block instead); reserved (written as 1).  The generator stops unless
 *                        every other count is non-zero, and that one in the three records of the second tiling.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbEncInterPrediction.h"
#include "EbInterPrediction.h"
#include "EbModeDecisionProcess.h"
#include "EbWarpedMotion.h"
#include "EbUtility.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "golden_io.h"

typedef void (*Warp8Fn)(const int32_t *, const uint8_t *, int, int, int, uint8_t *, int, int, int, int, int, int, int, ConvolveParams *,
                        int16_t, int16_t, int16_t, int16_t);
typedef void (*Warp16Fn)(const int32_t *, const uint8_t *, const uint8_t *, int, int, int, int, uint16_t *, int, int, int, int, int, int,
                         int, int, ConvolveParams *, int16_t, int16_t, int16_t, int16_t);
/* the reference's AVX2 forms (common_dsp_rtcd.h declares them only under ARCH_X86_64); weak: absent from a C-only link */
__attribute__((weak)) void svt_av1_warp_affine_avx2(const int32_t *, const uint8_t *, int, int, int, uint8_t *, int, int, int, int, int, int,
                                                    int, ConvolveParams *, int16_t, int16_t, int16_t, int16_t);
__attribute__((weak)) void svt_av1_highbd_warp_affine_avx2(const int32_t *, const uint8_t *, const uint8_t *, int, int, int, int,
                                                           uint16_t *, int, int, int, int, int, int, int, int, ConvolveParams *, int16_t,
                                                           int16_t, int16_t, int16_t);
static Warp8Fn  g_warp8[2]  = {svt_av1_warp_affine_c, svt_av1_warp_affine_avx2};
static Warp16Fn g_warp16[2] = {svt_av1_highbd_warp_affine_c, svt_av1_highbd_warp_affine_avx2};
static void     bind_warp(int pass) { svt_av1_warp_affine = g_warp8[pass], svt_av1_highbd_warp_affine = g_warp16[pass]; }
static int      g_simd;

static uint32_t draw(uint64_t seed, uint64_t i, uint32_t mod) {
    Rng r = {seed + i * 0x9E3779B97F4A7C15ull};
    return (uint32_t)(rng_next(&r) % mod);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

static GoldenFile *g_file;
static const char *nm(const char *fmt, int i, int a) {
    static char s[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(s[k], sizeof s[k], fmt, i, a);
    return s[k];
}
static void put(const char *name, char dt, int ndim, uint32_t d0, uint32_t d1, const void *data) {
    uint32_t dims[4] = {d0, d1, 0, 0};
    golden_put(g_file, name, dt, ndim, dims, data);
}
static void put_plane(const char *name, int bd, int h, int w, const uint16_t *a) {
    uint8_t *t8 = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++) t8[i] = (uint8_t)a[i];
    put(name, bd > 8 ? 'H' : 'B', 2, h, w, bd > 8 ? (const void *)a : (const void *)t8);
    free(t8);
}

static int shear(const int32_t mat[6], int16_t abgd[4]) {
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof wm);
    memcpy(wm.wmmat, mat, sizeof wm.wmmat);
    const int r = svt_get_shear_params(&wm);
    abgd[0] = wm.alpha, abgd[1] = wm.beta, abgd[2] = wm.gamma, abgd[3] = wm.delta;
    return r;
}

/* ---- tables ---- */
static void gen_tables(void) {
    int32_t lut[257];
    put("filter", 'h', 2, 193, 8, svt_aom_warped_filter);
    for (int f = 0; f <= 256; f++) {
        int32_t mat[6] = {0, 0, f < 256 ? 256 + f : 1023, 2048, f < 256 ? 2048 : 4096, 0};
        int     c;
        for (c = 8192 - 40; c <= 16384; c++) {
            int16_t abgd[4];
            mat[5] = 65536 + c;
            shear(mat, abgd);
            if (abgd[3] == 0) break;
        }
        lut[f] = c + 31;
    }
    put("div_lut", 'i', 1, 257, 0, lut);
}

/* ---- shear ---- */
static void gen_shear(void) {
    enum { N = 320 };
    static int32_t in[N][6], out[N][5];
    int32_t        kinds[12] = {0};
    const int      one = 1 << 16;
    static const int32_t fixed[][6] = {
        {0, 0, 0, 0, 0, 65536},           {0, 0, -65536, 0, 0, 65536},       {5 << 16, -(3 << 16), 65536, 0, 0, 65536},
        {12345, -54321, 65536, 0, 0, 65536}, {0, 0, 65536 + 16320, 0, 0, 65536}, {0, 0, 65536 + 16384, 0, 0, 65536},
        {0, 0, 65536 - 16320, 0, 0, 65536}, {0, 0, 65536 - 16384, 0, 0, 65536}, {0, 0, 65536, 9344, 0, 65536},
        {0, 0, 65536, 9408, 0, 65536},    {0, 0, 65536, -9344, 0, 65536},    {0, 0, 65536, -9408, 0, 65536},
        {0, 0, 65536, 0, 8192, 65536 + 8128}, {0, 0, 65536, 0, 8192, 65536 + 8192}, {0, 0, 65536, 0, -8192, 65536 - 8128},
        {0, 0, 65536, 0, -8192, 65536 - 8192}, {0, 0, 65536 + 40000, 0, 0, 65536}, {0, 0, 1, 0, 0, 65536},
        {0, 0, 65536, 40000, 0, 65536},   {0, 0, 65536, -40000, 0, 65536},   {0, 0, 65536, 0, 40000, 65536},
        {0, 0, 65536, 0, -40000, 65536},  {0, 0, 65536, 0, 0, 65536 + 40000}, {0, 0, 65536, 0, 0, 65536 - 40000},
        {0, 0, 65536 - 900, -700, -650, 65536 - 800}, {0, 0, 1, 2000000000, 2000000000, 65536}, {0, 0, 3, 0, -2000000000, 0},
        {0, 0, 2147483647, 0, 0, 65536},  {0, 0, 65536 + 32, 32, 32, 65536 + 32}, {0, 0, 65536 + 31, -31, 31, 65536 - 31},
        {0, 0, 65536 - 32, -32, -32, 65536 - 32}};
    const int nf = (int)(sizeof fixed / sizeof fixed[0]);
    Rng       r = {0x5750000000200000ull};
    for (int i = 0; i < N; i++) {
        if (i < nf) {
            memcpy(in[i], fixed[i], sizeof in[i]);
        } else {
            /* deviations of growing size, of either sign; every eighth model has a small or negative wmmat[2] */
            const int s = 1 << (4 + (i % 13));
            in[i][0] = (int32_t)rng_below(&r, 1 << 24) - (1 << 23), in[i][1] = (int32_t)rng_below(&r, 1 << 24) - (1 << 23);
            in[i][2] = one + (int32_t)rng_below(&r, 2 * s + 1) - s, in[i][3] = (int32_t)rng_below(&r, 2 * s + 1) - s;
            in[i][4] = (int32_t)rng_below(&r, 2 * s + 1) - s, in[i][5] = one + (int32_t)rng_below(&r, 2 * s + 1) - s;
            if (i % 8 == 7) in[i][2] = (int32_t)rng_below(&r, 4001) - 2000;
        }
        int16_t abgd[4];
        out[i][0] = shear(in[i], abgd);
        for (int k = 0; k < 4; k++) out[i][1 + k] = abgd[k];
        const int32_t *m = in[i];
        const int      l1 = 4 * abs(abgd[0]) + 7 * abs(abgd[1]), l2 = 4 * abs(abgd[2]) + 4 * abs(abgd[3]);
        kinds[0] += m[2] <= 0;
        kinds[1] += m[2] == one && !m[3] && !m[4] && m[5] == one && out[i][0] == 1;
        if (m[2] > 0) {
            kinds[2] += out[i][0] == 1 && l1 + 4 * 64 >= 65536, kinds[3] += out[i][0] == 0 && l1 >= 65536 && l1 - 7 * 64 < 65536;
            kinds[4] += out[i][0] == 1 && l2 + 4 * 64 >= 65536, kinds[5] += out[i][0] == 0 && l2 >= 65536 && l2 - 4 * 64 < 65536;
            for (int k = 0; k < 4; k++) kinds[6 + k] += abgd[k] == -32768;
            kinds[10] += out[i][0] == 1 && abgd[0] < 0 && abgd[1] < 0 && abgd[2] < 0 && abgd[3] < 0;
        }
        kinds[11]++;
    }
    for (int k = 0; k < 12; k++)
        if (!kinds[k]) fprintf(stderr, "shear: nothing of kind %d\n", k), exit(3);
    put("shear_in", 'i', 2, N, 6, in);
    put("shear_out", 'i', 2, N, 5, out);
    put("shear_kinds", 'i', 1, 12, 0, kinds);
}

/* ---- unit records ---- */
#define FR(px, f) (((px) * 65536) + (f))
static const int32_t g_models[][6] = {
    {FR(3, 0x8000), FR(2, 0x4000), 65536, 0, 0, 65536},         /* identity, fractional translation */
    {FR(2, 0xFFFF), FR(1, 0), 65536 + 16320, 0, 0, 65536},      /* alpha at its largest, either sign */
    {FR(1, 0), FR(3, 0xFFFF), 65536 - 16320, 0, 0, 65536},
    {FR(4, 0xFFC0), FR(2, 0x1000), 65536, 9344, 0, 65536},      /* beta */
    {FR(4, 0x0000), FR(2, 0xF000), 65536, -9344, 0, 65536},
    {FR(2, 0x2000), FR(3, 0xFFC0), 65536, 0, 16320, 65536},     /* gamma */
    {FR(2, 0xE000), FR(3, 0x0000), 65536, 0, -16320, 65536},
    {FR(1, 0x3000), FR(1, 0xFFFF), 65536, 0, 0, 65536 + 16320}, /* delta */
    {FR(5, 0xD000), FR(4, 0x0000), 65536, 0, 0, 65536 - 16320},
    {FR(-20, 0x5000), FR(1, 0x2000), 65536 + 640, -320, 256, 65536 - 512}, /* the origin left of the plane by more than 7 */
    {FR(60, 0x5000), FR(1, 0x2000), 65536 - 640, 320, -256, 65536 + 512},  /* right */
    {FR(2, 0x7000), FR(-24, 0x9000), 65536 + 128, 448, 192, 65536 + 64},   /* above */
    {FR(2, 0x7000), FR(40, 0x9000), 65536 - 128, -448, -192, 65536 - 64},  /* below */
    {FR(-100, 0x0400), FR(0, 0), 65536, 0, 0, 65536},           /* by more than the plane's size */
    {FR(100, 0x0400), FR(0, 0), 65536, 0, 0, 65536},
    {FR(0, 0), FR(-100, 0xFC00), 65536, 0, 0, 65536},
    {FR(0, 0), FR(100, 0xFC00), 65536, 0, 0, 65536},
    /* pure translation onto the table's heaviest row: gen_units' extreme records (below) */
    {FR(3, 0x7400), FR(2, 0x7400), 65536, 0, 0, 65536},
    /* the last two: the largest beta and gamma at once; gen_units sets their translation so that the first unit's projected
     * centre has fraction 0 (filter row 0 of both passes) and 65535 (row 192 of the horizontal pass, 176 of the vertical
     * one, which spans 8 rows, not 15, and cannot reach further) */
    {0, 0, 65536, 9344, 16320, 65536 + 2327},
    {0, 0, 65536, 9344, 16320, 65536 + 2327}};
#define N_MODELS ((int)(sizeof g_models / sizeof g_models[0]))

#define HEAVY_MODEL (N_MODELS - 3)

static int32_t g_unit_kinds[16];
static int32_t g_tmp[3][2] = {{1 << 30, -1}, {1 << 30, -1}, {1 << 30, -1}}; /* per bit depth 8, 10, 12: min, max of the intermediate */
/* What a call reaches, by the index arithmetic and the horizontal pass of the C restated: the filter rows, where the
 * projected origin lies against the plane, and the extremes of the horizontal intermediate (the C's tmp[]) */
static void count_call(int bd, const int32_t *mat, const int16_t *abgd, const uint16_t *plane, int w, int h, int p_col, int p_row, int pw,
                       int ph, int ss) {
    const int rbh = bd == 8 ? 3 : 3 + (bd - 10), bi = bd == 8 ? 0 : bd == 10 ? 1 : 2; /* get_conv_params_no_round's round_0 */
    for (int i = p_row; i < p_row + ph; i += 8)
        for (int j = p_col; j < p_col + pw; j += 8) {
            const int32_t sx_ = (j + 4) << ss, sy_ = (i + 4) << ss;
            const int32_t x4 = (mat[2] * sx_ + mat[3] * sy_ + mat[0]) >> ss, y4 = (mat[4] * sx_ + mat[5] * sy_ + mat[1]) >> ss;
            const int     ix4 = x4 >> 16, iy4 = y4 >> 16;
            const int     sx4 = ((x4 & 65535) + abgd[0] * -4 + abgd[1] * -4) & ~63, sy4 = ((y4 & 65535) + abgd[2] * -4 + abgd[3] * -4) & ~63;
            g_unit_kinds[8] += ix4 <= -7, g_unit_kinds[9] += ix4 >= w + 6, g_unit_kinds[10] += iy4 <= -7, g_unit_kinds[11] += iy4 >= h + 6;
            g_unit_kinds[12] += ix4 <= -w, g_unit_kinds[13] += ix4 >= 2 * w, g_unit_kinds[14] += iy4 <= -h, g_unit_kinds[15] += iy4 >= 2 * h;
            for (int k = 0; k < 15; k++)
                for (int l = 0; l < 8; l++) {
                    const int      o = ((sx4 + abgd[1] * (k - 3) + abgd[0] * l + 512) >> 10) + 64, iy = clampi(iy4 + k - 7, 0, h - 1);
                    const int16_t *c = svt_aom_warped_filter[o];
                    int32_t        sum = 1 << (bd + 6);
                    for (int m = 0; m < 8; m++) sum += plane[iy * w + clampi(ix4 + l - 7 + m, 0, w - 1)] * c[m];
                    sum = (sum + ((1 << rbh) >> 1)) >> rbh;
                    if (sum < g_tmp[bi][0]) g_tmp[bi][0] = sum;
                    if (sum > g_tmp[bi][1]) g_tmp[bi][1] = sum;
                    g_unit_kinds[0] += o == 0, g_unit_kinds[1] += o == 192;
                }
            for (int k = 0; k < 8; k++)
                for (int l = 0; l < 8; l++) {
                    const int o = ((sy4 + abgd[3] * k + abgd[2] * l + 512) >> 10) + 64;
                    g_unit_kinds[2] += o == 0, g_unit_kinds[3] += o == 176;
                }
        }
}
static void fill_plane(uint16_t *p, int bd, int w, int h, int content, uint64_t seed, int inverse) {
    const int maxv = (1 << (bd > 10 ? 10 : bd)) - 1; /* the split 8 + 2 layout holds ten bits, whatever bd says */
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            p[y * w + x] = (uint16_t)(content == 0   ? draw(seed, (uint64_t)y * w + x, maxv + 1)
                                      : content == 1 ? 0
                                      : content == 2 ? maxv
                                      : ((svt_aom_warped_filter[96][(content == 3 ? x : y) & 7] > 0) ^ inverse) ? maxv : 0);
}
/* one call of the C (pass 0) or AVX2 (pass 1) function on a w x h plane of 16-bit working samples */
static void warp_call(int pass, int bd, const int32_t *mat, const int16_t *abgd, const uint16_t *plane, int w, int h, uint16_t *pred,
                      int p_col, int p_row, int pw, int ph, int ss, ConvolveParams *cp) {
    uint8_t *p8 = malloc((size_t)w * h), *p2 = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++)
        p8[i] = (uint8_t)(bd > 8 ? plane[i] >> 2 : plane[i]), p2[i] = (uint8_t)(bd > 8 ? (plane[i] & 3) << 6 : 0);
    if (bd == 8) {
        uint8_t *o8 = malloc((size_t)pw * ph);
        for (int i = 0; i < pw * ph; i++) o8[i] = (uint8_t)pred[i];
        g_warp8[pass](mat, p8, w, h, w, o8, p_col, p_row, pw, ph, pw, ss, ss, cp, abgd[0], abgd[1], abgd[2], abgd[3]);
        for (int i = 0; i < pw * ph; i++) pred[i] = o8[i];
        free(o8);
    } else {
        g_warp16[pass](mat, p8, p2, w, h, w, w, pred, p_col, p_row, pw, ph, pw, ss, ss, bd, cp, abgd[0], abgd[1], abgd[2], abgd[3]);
    }
    free(p8), free(p2);
}
static int g_seen[3][3], g_seen_ss[2], g_seen_size[4], g_clip[3][2];
static const int g_sizes[4][2] = {{8, 8}, {8, 16}, {16, 8}, {32, 8}}, g_bds[3] = {8, 10, 12};
/* one unit record: `flip` inverts the pattern contents of both passes (pass 1 is always the inverse of pass 0) */
static void unit_record(int n, int content, int mi, int m2, int bi, int sz, int mode, int ss, int small, int p_col, int p_row, int flip) {
    const int bd = g_bds[bi], w = small ? 12 : 40, h = small ? 10 : 24, pw = g_sizes[sz][0], ph = g_sizes[sz][1];
    const int fwd = 4 + 3 * (n % 4), bck = 16 - fwd; /* 4 / 12, 7 / 9, 10 / 6, 13 / 3 */
    int16_t   abgd[2][4];
    int32_t   mm[2][6];
    for (int s = 0; s < 2; s++) {
        const int idx = s ? m2 : mi;
        memcpy(mm[s], g_models[idx], sizeof mm[s]);
        if (idx >= N_MODELS - 2) { /* fraction 0 or 65535 at the first unit's centre */
            const int32_t sx_ = (p_col + 4) << ss, sy_ = (p_row + 4) << ss, last = idx == N_MODELS - 1;
            mm[s][0] = ((p_col + 4) << (16 + ss)) - (mm[s][2] * sx_ + mm[s][3] * sy_) - last;
            mm[s][1] = ((p_row + 4) << (16 + ss)) - (mm[s][4] * sx_ + mm[s][5] * sy_) - last;
        }
    }
    if (shear(mm[0], abgd[0]) != 1 || shear(mm[1], abgd[1]) != 1) fprintf(stderr, "unit model %d or %d refused\n", mi, m2), exit(3);
    uint16_t *plane = malloc(sizeof(uint16_t) * w * h), out[32 * 16], out2[32 * 16], conv[32 * 16], conv2[32 * 16];
    const uint64_t seed = 0x5750000000000000ull + 16 * (uint64_t)n;
    g_seen[bi][mode] = 1, g_seen_ss[ss] = 1, g_seen_size[sz] = 1;
    for (int pass = 0; pass <= g_simd; pass++) {
        uint16_t      *o = pass ? out2 : out, *c = pass ? conv2 : conv;
        ConvolveParams cp = get_conv_params_no_round(0, 0, 0, c, pw, mode != 0, bd);
        memset(o, 0xA5, sizeof out), memset(c, 0x5A, sizeof conv);
        fill_plane(plane, bd, w, h, content, seed, flip);
        warp_call(pass, bd, mm[0], abgd[0], plane, w, h, o, p_col, p_row, pw, ph, ss, &cp);
        if (!pass) count_call(bd, mm[0], abgd[0], plane, w, h, p_col, p_row, pw, ph, ss);
        if (mode) {
            cp.do_average = 1, cp.use_jnt_comp_avg = mode == 2, cp.fwd_offset = fwd, cp.bck_offset = bck;
            fill_plane(plane, bd, w, h, content, seed + 8, !flip);
            warp_call(pass, bd, mm[1], abgd[1], plane, w, h, o, p_col, p_row, pw, ph, ss, &cp);
            if (!pass) count_call(bd, mm[1], abgd[1], plane, w, h, p_col, p_row, pw, ph, ss);
        }
    }
    if (g_simd && (memcmp(out, out2, sizeof(uint16_t) * pw * ph) || (mode && memcmp(conv, conv2, sizeof(uint16_t) * pw * ph))))
        fprintf(stderr, "avx2 != c: unit record %d (%dx%d, %d bits, mode %d)\n", n, pw, ph, bd, mode), exit(3);
    for (int i = 0; i < pw * ph; i++) {
        g_unit_kinds[4] += out[i] == 0, g_unit_kinds[5] += out[i] == (1 << bd) - 1;
        g_clip[bi][0] |= out[i] == 0, g_clip[bi][1] |= out[i] == (1 << bd) - 1;
    }
    if (mode) g_unit_kinds[6] += content == 3, g_unit_kinds[7] += content == 4;
    int32_t par[16] = {bd, w, h, p_col, p_row, pw, ph, ss, mode, content, mi, m2, fwd, bck, n, flip}, mats[2][6], sh[2][4];
    memcpy(mats, mm, sizeof mats);
    for (int k = 0; k < 8; k++) sh[k >> 2][k & 3] = abgd[k >> 2][k & 3];
    put(nm("u%d_par", n, 0), 'i', 1, 16, 0, par);
    put(nm("u%d_mat", n, 0), 'i', 2, 2, 6, mats);
    put(nm("u%d_abgd", n, 0), 'i', 2, 2, 4, sh);
    put_plane(nm("u%d_out", n, 0), bd, ph, pw, out);
    if (mode) put(nm("u%d_conv", n, 0), 'H', 2, ph, pw, conv);
    free(plane);
}
static int gen_units(void) {
    int n = 0;
    for (int content = 0; content < 5; content++)
        for (int mi = 0; mi < N_MODELS; mi++, n++) {
            const int small = n % 5 == 4;
            unit_record(n, content, mi, (mi + 3) % N_MODELS, n % 3, (n / 3) % 4, (n / 3 + n / 12) % 3, (n / 5) & 1, small,
                        small ? 0 : 8 * ((n / 7) & 1), small ? 0 : 8 * ((n / 11) & 1), 0);
        }
    /* The extreme records: the pattern contents under a pure translation whose fraction selects the table's heaviest row
     * (the largest sum of positive taps and the smallest of negative ones; its signs are the half-sample row's), inside the
     * plane, so that the lane whose window is in phase with the pattern gets every positive tap on max and every negative
     * one on zero, or the inverse.  Columns: the horizontal intermediate's two ends.  Rows: the vertical sum's, and with
     * them both clips of the output.  One compound record per depth carries both ends in its two passes. */
    for (int bi = 0; bi < 3; bi++) {
        static const int ex[5][3] = {{3, 0, 0}, {3, 0, 1}, {4, 0, 0}, {4, 0, 1}, {3, 1, 0}}; /* content, mode, flip */
        for (int e = 0; e < 5; e++, n++) unit_record(n, ex[e][0], HEAVY_MODEL, HEAVY_MODEL, bi, 2, ex[e][1], 0, 0, 8, 8, ex[e][2]);
    }
    /* the analytic ends of the intermediate: every positive (negative) tap of the heaviest row on max, the others on zero */
    int pos = 0, neg = 0, heavy = 0;
    for (int r = 0; r < 193; r++) {
        int p = 0, q = 0;
        for (int m = 0; m < 8; m++) p += svt_aom_warped_filter[r][m] > 0 ? svt_aom_warped_filter[r][m] : 0, q += svt_aom_warped_filter[r][m] < 0 ? svt_aom_warped_filter[r][m] : 0;
        if (p > pos) pos = p, heavy = r;
        if (q < neg) neg = q;
    }
    const int hx = ((g_models[HEAVY_MODEL][0] & 65535) + 512 >> 10) + 64;
    for (int m = 0; m < 8; m++)
        if ((svt_aom_warped_filter[heavy][m] > 0) != (svt_aom_warped_filter[96][m] > 0)) fprintf(stderr, "row %d has other signs than row 96\n", heavy), exit(3);
    int neg_heavy = 0;
    for (int m = 0; m < 8; m++) neg_heavy += svt_aom_warped_filter[heavy][m] < 0 ? svt_aom_warped_filter[heavy][m] : 0;
    if (hx != heavy || neg_heavy != neg) fprintf(stderr, "the heaviest row is %d (negative taps %d of %d), the extreme model selects %d\n", heavy, neg_heavy, neg, hx), exit(3);
    int32_t ends[3][4];
    for (int bi = 0; bi < 3; bi++) {
        const int bd = g_bds[bi], maxv = (1 << (bd > 10 ? 10 : bd)) - 1, rbh = bd == 8 ? 3 : 3 + (bd - 10), half = (1 << rbh) >> 1;
        const int lo = ((1 << (bd + 6)) + neg * maxv + half) >> rbh, hi = ((1 << (bd + 6)) + pos * maxv + half) >> rbh;
        if (g_tmp[bi][0] != lo || g_tmp[bi][1] != hi)
            fprintf(stderr, "%d bits: the intermediate spans [%d, %d], its analytic ends are [%d, %d]\n", bd, g_tmp[bi][0], g_tmp[bi][1], lo, hi), exit(3);
        if (hi >= 1 << 16) fprintf(stderr, "%d bits: the intermediate does not fit 16 bits\n", bd), exit(3);
        /* ten-bit samples cannot reach the upper clip of a 12-bit output */
        if (!g_clip[bi][0] || (bd <= 10 && !g_clip[bi][1])) fprintf(stderr, "%d bits: an output clip is not reached\n", bd), exit(3);
        ends[bi][0] = g_tmp[bi][0], ends[bi][1] = g_tmp[bi][1], ends[bi][2] = neg, ends[bi][3] = pos;
    }
    for (int k = 0; k < 9; k++)
        if (!g_seen[k / 3][k % 3]) fprintf(stderr, "units: no %d-bit record of mode %d\n", g_bds[k / 3], k % 3), exit(3);
    if (!g_seen_ss[0] || !g_seen_ss[1] || !g_seen_size[0] || !g_seen_size[1] || !g_seen_size[2] || !g_seen_size[3]) fprintf(stderr, "units: a size or subsampling is missing\n"), exit(3);
    for (int k = 0; k < 16; k++)
        if (!g_unit_kinds[k]) fprintf(stderr, "units: nothing of kind %d\n", k), exit(3);
    int32_t nn = n;
    put("nunit", 'i', 1, 1, 0, &nn);
    put("unit_kinds", 'i', 1, 16, 0, g_unit_kinds);
    put("unit_tmp", 'i', 2, 3, 4, ends);
    return n;
}

/* ---- batch records ---- */
static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static PictureControlSet       *g_pcs;
static void                     setup_reference(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
    bind_warp(0);
    svt_aom_build_blk_geom(GEOM_7);
    g_scs = calloc(1, sizeof *g_scs), g_ppcs = calloc(1, sizeof *g_ppcs), g_pcs = calloc(1, sizeof *g_pcs);
    g_pcs->ppcs = g_ppcs, g_pcs->scs = g_scs, g_ppcs->scs = g_scs, g_ppcs->is_not_scaled = 1;
    g_scs->seq_header.sb_size = BLOCK_128X128;
    g_scs->seq_header.order_hint_info.enable_order_hint = 1;
    g_scs->seq_header.order_hint_info.order_hint_bits   = 7;
    g_ppcs->cur_order_hint = 40, g_ppcs->ref_order_hint[LAST_FRAME - 1] = 37, g_ppcs->ref_order_hint[BWDREF_FRAME - 1] = 42;
}
typedef struct RefPic {
    uint8_t *p8[3], *p2[3];
} RefPic;
static void ref_alloc(RefPic *r, int bd, int w, int h, uint64_t seed) {
    const int sc = 1 << (bd - 8);
    for (int p = 0; p < 3; p++) {
        const int pw = w >> (p > 0), ph = h >> (p > 0);
        r->p8[p] = malloc((size_t)pw * ph), r->p2[p] = malloc((size_t)pw * ph);
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                const int v = clampi((2 * x + y) * sc / 4 + (int)draw(seed + p, (uint64_t)y * pw + x, 64 * sc), 0, (1 << bd) - 1);
                r->p8[p][y * pw + x] = (uint8_t)(bd > 8 ? v >> 2 : v), r->p2[p][y * pw + x] = (uint8_t)(bd > 8 ? (v & 3) << 6 : 0);
            }
    }
}
static void ref_desc(EbPictureBufferDesc *d, const RefPic *r, int bd, int w, int h) {
    memset(d, 0, sizeof *d);
    d->buffer_y = r->p8[0], d->buffer_cb = r->p8[1], d->buffer_cr = r->p8[2];
    d->buffer_bit_inc_y = r->p2[0], d->buffer_bit_inc_cb = r->p2[1], d->buffer_bit_inc_cr = r->p2[2];
    d->width = (uint16_t)w, d->height = (uint16_t)h;
    d->stride_y = d->stride_bit_inc_y = (uint16_t)w;
    d->stride_cb = d->stride_bit_inc_cb = d->stride_cr = d->stride_bit_inc_cr = (uint16_t)(w / 2);
}
typedef struct Block {
    int     x, y, w, h, ref0, ref1, dist_wtd, fwd, bck, mds; /* mds: the block geometry's index + 1, looked up once */
    int32_t mat[2][6];
} Block;
static const int g_t1[][4] = {{0, 0, 64, 64},   {64, 0, 16, 64},  {80, 0, 16, 16},  {96, 0, 32, 8},   {96, 8, 8, 32},   {104, 8, 8, 8},
                              {112, 8, 16, 16}, {0, 88, 8, 8},    {120, 88, 8, 8},  {0, 64, 32, 8},   {32, 64, 32, 32}, {64, 64, 16, 16},
                              {80, 64, 16, 16}, {96, 64, 8, 8},   {104, 16, 8, 32}, {112, 24, 16, 16}, {80, 16, 16, 16}, {80, 32, 16, 16},
                              {8, 88, 8, 8},    {112, 88, 8, 8},  {0, 72, 16, 16}};
static const int g_t2[][4] = {{0, 32, 128, 64}, {0, 0, 32, 8},    {32, 0, 8, 32},   {40, 0, 8, 8},    {48, 0, 16, 16},  {64, 0, 16, 16},
                              {80, 0, 8, 32},   {88, 0, 8, 8},    {96, 0, 32, 8},   {96, 8, 16, 16},  {112, 8, 16, 16}, {0, 8, 32, 8},
                              {0, 16, 16, 16},  {16, 16, 16, 16}, {40, 8, 8, 8},    {48, 16, 16, 16}, {64, 16, 16, 16}, {88, 8, 8, 8},
                              {88, 16, 8, 8},   {88, 24, 8, 8},   {40, 16, 8, 16}};
#define N_BLOCKS 21
static void draw_model(int32_t *m, Rng *r, int k) {
    m[2] = 65536 + (int32_t)rng_below(r, 4001) - 2000, m[3] = (int32_t)rng_below(r, 3001) - 1500;
    m[4] = (int32_t)rng_below(r, 3001) - 1500, m[5] = 65536 + (int32_t)rng_below(r, 4001) - 2000;
    m[0] = ((int32_t)rng_below(r, 17) - 8) * 65536 + (int32_t)rng_below(r, 65536);
    m[1] = ((int32_t)rng_below(r, 17) - 8) * 65536 + (int32_t)rng_below(r, 65536);
    switch (k % 7) { /* every seventh block of each kind leaves the picture on one side */
    case 1: m[0] -= 200 << 16; break;
    case 2: m[0] += 200 << 16; break;
    case 3: m[1] -= 200 << 16; break;
    case 4: m[1] += 200 << 16; break;
    default: break;
    }
}
static uint32_t find_mds(int w, int h) {
    for (uint32_t k = 0; k < MAX_NUM_BLOCKS_ALLOC; k++) {
        const BlockGeom *g = get_blk_geom_mds(k);
        if (g->bwidth == w && g->bheight == h && g->has_uv) return k;
    }
    fprintf(stderr, "no block geometry of %dx%d\n", w, h), exit(3);
}
static void predict_batch(int bd, int w, int h, int chroma, RefPic *refs, Block *blocks, int n, uint16_t *pred[3]) {
    EbPictureBufferDesc rd[3], pd;
    const int           hbd = bd > 8;
    uint8_t            *pb[3];
    for (int r = 0; r < 3; r++) ref_desc(&rd[r], &refs[r], bd, w, h);
    memset(&pd, 0, sizeof pd);
    for (int p = 0; p < 3; p++) pb[p] = calloc((size_t)(w >> (p > 0)) * (h >> (p > 0)), hbd ? 2 : 1);
    pd.buffer_y = pb[0], pd.buffer_cb = pb[1], pd.buffer_cr = pb[2];
    pd.stride_y = (uint16_t)w, pd.stride_cb = pd.stride_cr = (uint16_t)(w / 2), pd.width = (uint16_t)w, pd.height = (uint16_t)h;
    MvReferenceFrame rf[2] = {LAST_FRAME, BWDREF_FRAME}, rf1[2] = {LAST_FRAME, NONE_FRAME};
    for (int k = 0; k < n; k++) {
        Block                 *b = &blocks[k];
        const int              two = b->ref1 != 255;
        BlkStruct              blk;
        MacroBlockD            xd;
        MvUnit                 mvu;
        InterInterCompoundData comp;
        EbWarpedMotionParams   wm[2];
        memset(&blk, 0, sizeof blk), memset(&xd, 0, sizeof xd), memset(&comp, 0, sizeof comp), memset(&mvu, 0, sizeof mvu), memset(wm, 0, sizeof wm);
        if (!b->mds) b->mds = 1 + (int)find_mds(b->w, b->h);
        blk.av1xd = &xd, blk.mds_idx = (uint16_t)(b->mds - 1);
        mvu.pred_direction = two ? BI_PRED : UNI_PRED_LIST_0;
        comp.type          = b->dist_wtd ? COMPOUND_DISTWTD : COMPOUND_AVERAGE;
        for (int r = 0; r < 1 + two; r++) {
            memcpy(wm[r].wmmat, b->mat[r], sizeof wm[r].wmmat);
            wm[r].wmtype = AFFINE;
            if (!svt_get_shear_params(&wm[r])) fprintf(stderr, "block %d: model %d refused\n", k, r), exit(3);
        }
        const int small = b->w < 16 || b->h < 16;
        svt_aom_warped_motion_prediction(g_pcs, &mvu, (uint8_t)av1_ref_frame_type(two ? rf : rf1), (uint8_t)(b->dist_wtd ? 0 : 1), &comp,
                                         (uint16_t)b->x, (uint16_t)b->y, &blk, get_blk_geom_mds(blk.mds_idx), &rd[b->ref0],
                                         two ? &rd[b->ref1] : NULL, &pd, (uint16_t)b->x, (uint16_t)b->y, NULL, NULL, NULL, NULL, &wm[0],
                                         &wm[1], (uint8_t)bd,
                                         chroma && !small ? PICTURE_BUFFER_DESC_FULL_MASK : PICTURE_BUFFER_DESC_LUMA_MASK,
                                         1 /* the encode pass: inter-intra is read from blk (off), not from a candidate */);
    }
    for (int p = 0; p < 3; p++) {
        const size_t cnt = (size_t)(w >> (p > 0)) * (h >> (p > 0));
        for (size_t i = 0; i < cnt; i++) pred[p][i] = hbd ? ((uint16_t *)pb[p])[i] : pb[p][i];
        free(pb[p]);
    }
}
static void count_blocks(int32_t kinds[24], const Block *bl, int n, int w, int h) {
    for (int k = 0; k < n; k++) {
        const Block *b = &bl[k];
        const int    two = b->ref1 != 255;
        kinds[0] += b->w == 8 && b->h == 8, kinds[1] += b->h == 4 * b->w, kinds[2] += b->w == 4 * b->h;
        kinds[3] += b->w == 16 && b->h == 16, kinds[4] += b->w >= 64 && b->h >= 64;
        if (k) kinds[5] += two != (bl[k - 1].ref1 != 255);
        kinds[6] += two && !b->dist_wtd, kinds[7] += two && b->dist_wtd;
        kinds[8] += two && b->ref0 == b->ref1 && !memcmp(b->mat[0], b->mat[1], sizeof b->mat[0]);
        kinds[9] += !b->x && !b->y, kinds[10] += b->x + b->w == w && !b->y, kinds[11] += !b->x && b->y + b->h == h;
        kinds[12] += b->x + b->w == w && b->y + b->h == h, kinds[13] += b->w < 16 || b->h < 16, kinds[20] += !two, kinds[22] += b->w == 128 && b->h == 64;
        int edge[4] = {0}, neg[2] = {0};
        for (int r = 0; r < 1 + two; r++)
            for (int i = b->y; i < b->y + b->h; i += 8)
                for (int j = b->x; j < b->x + b->w; j += 8) {
                    const int32_t *m = b->mat[r];
                    const int32_t  dx = m[2] * (j + 4) + m[3] * (i + 4) + m[0], dy = m[4] * (j + 4) + m[5] * (i + 4) + m[1];
                    const int      ix4 = dx >> 16, iy4 = dy >> 16;
                    edge[0] |= ix4 - 7 < 0, edge[1] |= ix4 + 7 > w - 1, edge[2] |= iy4 - 7 < 0, edge[3] |= iy4 + 7 > h - 1;
                    neg[0] |= dx < 0, neg[1] |= dy < 0;
                }
        for (int e = 0; e < 4; e++) kinds[14 + e] += edge[e];
        kinds[18] += neg[0], kinds[19] += neg[1];
    }
    kinds[21] = n, kinds[23] = 1;
}
static void gen_batches(void) {
    /* {bd, chroma, tiling}: the 128x64 block (the second tiling) at both depths, with and without chroma */
    static const int cases[4][3] = {{8, 1, 0}, {10, 1, 1}, {10, 0, 1}, {8, 1, 1}};
    const int        w = 128, h = 96, nr = 3, n = N_BLOCKS;
    setup_reference();
    for (int i = 0; i < 4; i++) {
        const int    bd = cases[i][0], chroma = cases[i][1];
        const int(*t)[4] = cases[i][2] ? g_t2 : g_t1;
        static uint8_t cover[96][128];
        memset(cover, 0, sizeof cover);
        for (int k = 0; k < n; k++)
            for (int y = t[k][1]; y < t[k][1] + t[k][3]; y++)
                for (int x = t[k][0]; x < t[k][0] + t[k][2]; x++)
                    if (y >= h || x >= w || cover[y][x]++) fprintf(stderr, "record %d: block %d overlaps or leaves the picture\n", i, k), exit(3);
        Rng       r = {0x5750000000080000ull + i};
        Block     blocks[N_BLOCKS];
        RefPic    refs[3];
        uint16_t *pred[3], *again[3];
        int32_t   kinds[24] = {0}, par[8] = {bd, w, h, nr, chroma, n, i, 0};
        for (int k = 0; k < n; k++) {
            Block *b = &blocks[k];
            memset(b, 0, sizeof *b);
            b->x = t[k][0], b->y = t[k][1], b->w = t[k][2], b->h = t[k][3];
            b->ref0 = (int)rng_below(&r, nr), b->ref1 = (k % 3 == 1) ? 255 : (int)rng_below(&r, nr);
            b->dist_wtd = b->ref1 != 255 && (k & 1);
            draw_model(b->mat[0], &r, k), draw_model(b->mat[1], &r, k + 3);
            if (k == 5) b->ref1 = b->ref0, memcpy(b->mat[1], b->mat[0], sizeof b->mat[0]);
            if (k == 0) b->mat[0][0] = -(3 << 16) - 0x1234, b->mat[0][1] = -(2 << 16) - 0x4321; /* negative dst_x, dst_y at (0, 0) */
            if (b->ref1 == 255) memset(b->mat[1], 0, sizeof b->mat[1]);
            if (b->dist_wtd) {
                int fwd, bck, use;
                svt_av1_dist_wtd_comp_weight_assign(&g_scs->seq_header, g_ppcs->cur_order_hint, g_ppcs->ref_order_hint[LAST_FRAME - 1],
                                                    g_ppcs->ref_order_hint[BWDREF_FRAME - 1], 0, 0, &fwd, &bck, &use, 1);
                b->fwd = fwd, b->bck = bck;
                if (!use || fwd == bck) fprintf(stderr, "the distance weights are %d / %d\n", fwd, bck), exit(3);
            }
        }
        for (int k = 0; k < nr; k++) ref_alloc(&refs[k], bd, w, h, 0x5750000000100000ull + 256 * (uint64_t)i + 4 * k);
        for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2), again[p] = calloc((size_t)w * h, 2);
        predict_batch(bd, w, h, chroma, refs, blocks, n, pred);
        if (g_simd) {
            bind_warp(1);
            predict_batch(bd, w, h, chroma, refs, blocks, n, again);
            bind_warp(0);
            for (int p = 0; p < 3; p++)
                if (memcmp(again[p], pred[p], (size_t)w * h * 2)) fprintf(stderr, "avx2 != c: batch record %d plane %d\n", i, p), exit(3);
        }
        count_blocks(kinds, blocks, n, w, h);
        for (int k = 0; k < 24; k++)
            if (!kinds[k] && !(k == 22 && !cases[i][2])) fprintf(stderr, "batch record %d: nothing of kind %d\n", i, k), exit(3);
        int32_t rec[N_BLOCKS][22];
        for (int k = 0; k < n; k++) {
            const Block  *b = &blocks[k];
            const int32_t v[10] = {b->x, b->y, b->w, b->h, b->ref0, b->ref1, b->dist_wtd, b->fwd, b->bck, 0};
            memcpy(rec[k], v, sizeof v), memcpy(rec[k] + 10, b->mat[0], 24), memcpy(rec[k] + 16, b->mat[1], 24);
        }
        put(nm("q%d_par", i, 0), 'i', 1, 8, 0, par);
        put(nm("q%d_blocks", i, 0), 'i', 2, n, 22, rec);
        put(nm("q%d_kinds", i, 0), 'i', 1, 24, 0, kinds);
        for (int p = 0; p < (chroma ? 3 : 1); p++) put_plane(nm("q%d_pred%d", i, p), bd, h >> (p > 0), w >> (p > 0), pred[p]);
        for (int k = 0; k < nr; k++)
            for (int p = 0; p < 3; p++) free(refs[k].p8[p]), free(refs[k].p2[p]);
        for (int p = 0; p < 3; p++) free(pred[p]), free(again[p]);
    }
    int32_t nb = 4;
    put("nbatch", 'i', 1, 1, 0, &nb);
}

/* scripts/warp_perf.py's workloads through the reference's C on one core: the compound fixture's tiling (all 17 sizes, 23
 * blocks per 256 x 192) repeated over the picture, models drawn as the script draws them (translations within +-8 samples,
 * wmmat[2], [5] within 2000 and [3], [4] within 1500 of the identity), every block from one reference, then from two */
static const int g_perf_tiling[][4] = {
    {0, 0, 128, 128},   {128, 0, 128, 64},  {128, 64, 64, 128}, {192, 64, 64, 64},  {192, 128, 64, 32},  {192, 160, 32, 32},
    {224, 160, 32, 16}, {224, 176, 16, 16}, {240, 176, 8, 16},  {248, 176, 8, 8},   {248, 184, 8, 8},    {0, 128, 32, 64},
    {32, 128, 64, 32},  {32, 160, 64, 16},  {32, 176, 32, 8},   {32, 184, 32, 8},   {64, 176, 16, 16},   {80, 176, 16, 8},
    {80, 184, 16, 8},   {96, 128, 16, 64},  {112, 128, 16, 32}, {112, 160, 8, 32},  {120, 160, 8, 32}};
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static void time_reference(void) {
    static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
    setup_reference();
    for (int k = 0; k < 2; k++)
        for (int two = 0; two < 2; two++) {
            const int bd = shapes[k][0], w = shapes[k][1], h = shapes[k][2], cols = w / 256, rows = h / 192;
            Rng       r = {0x5750000000300000ull};
            Block    *blocks = calloc((size_t)cols * rows * 23, sizeof(Block));
            RefPic    refs[3];
            uint16_t *pred[3];
            int       n = 0;
            long long outputs = 0;
            for (int q = 0; q < cols * rows; q++)
                for (int j = 0; j < 23; j++, n++) {
                    Block *b = &blocks[n];
                    b->x = g_perf_tiling[j][0] + (q % cols) * 256, b->y = g_perf_tiling[j][1] + (q / cols) * 192;
                    b->w = g_perf_tiling[j][2], b->h = g_perf_tiling[j][3];
                    b->ref0 = (int)rng_below(&r, 3), b->ref1 = two ? (int)rng_below(&r, 3) : 255;
                    for (int m = 0; m < 1 + two; m++) {
                        int32_t *t = b->mat[m];
                        t[0] = (int32_t)rng_below(&r, 16 << 16) - (8 << 16), t[1] = (int32_t)rng_below(&r, 16 << 16) - (8 << 16);
                        t[2] = 65536 + (int32_t)rng_below(&r, 4001) - 2000, t[3] = (int32_t)rng_below(&r, 3001) - 1500;
                        t[4] = (int32_t)rng_below(&r, 3001) - 1500, t[5] = 65536 + (int32_t)rng_below(&r, 4001) - 2000;
                    }
                    outputs += (long long)b->w * b->h * (b->w >= 16 && b->h >= 16 ? 3 : 2) / 2; /* no chroma below 16 */
                }
            for (int q = 0; q < 3; q++) ref_alloc(&refs[q], bd, w, h, 0x5750000000400000ull + 4 * q);
            for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2);
            predict_batch(bd, w, h, 1, refs, blocks, n, pred); /* warm-up; looks the block geometries up */
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                const double t0 = now_ms();
                predict_batch(bd, w, h, 1, refs, blocks, n, pred);
                const double t1 = now_ms();
                if (t1 - t0 < best) best = t1 - t0;
            }
            printf("{\"workload\": \"%dx%d %d-bit, %d blocks over %dx%d, %d reference%s\", \"predict_c_ms\": %.2f, \"output_samples\": %lld, "
                   "\"ps_per_filtered_sample\": %.0f, \"reps\": 3}\n",
                   w, h, bd, n, cols * 256, rows * 192, 1 + two, two ? "s" : "", best, outputs, best * 1e9 / ((1 + two) * (double)outputs));
            for (int q = 0; q < 3; q++)
                for (int p = 0; p < 3; p++) free(refs[q].p8[p]), free(refs[q].p2[p]);
            for (int p = 0; p < 3; p++) free(pred[p]);
            free(blocks);
        }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    g_simd = __builtin_cpu_supports("avx2") && svt_av1_warp_affine_avx2 && svt_av1_highbd_warp_affine_avx2 ? 1 : 0;
    if (!strcmp(argv[1], "--time")) {
        time_reference();
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    gen_tables();
    gen_shear();
    const int nu = gen_units();
    gen_batches();
    golden_close(&g);
    fprintf(stderr, "tables, 320 shear records, %d unit records, 4 batch records; %s\n", nu,
            g_simd ? "every unit and batch record equal through the _avx2 functions" : "the _c functions only");
    return 0;
}
