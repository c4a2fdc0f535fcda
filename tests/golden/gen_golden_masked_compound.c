/*
 * gen_golden_masked_compound.c — writes tests/golden/masked_compound.bin: the reference's masked compound prediction: the
 * wedge masks of svt_av1_init_wedge_masks (EbInterPrediction.c:1445-2132), svt_av1_build_compound_diffwtd_mask_d16_c
 * (C_DEFAULT/EbInterPrediction_c.c:15-40), svt_aom_lowbd_blend_a64_d16_mask_c / svt_aom_highbd_blend_a64_d16_mask_c
 * (EbBlend_a64_mask.c:34-195) and svt_aom_inter_prediction with COMPOUND_WEDGE / COMPOUND_DIFFWTD
 * (EbEncInterPrediction.c:4070, :50-164) on deterministic inputs (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration) and the reference's AVX2 sources of the three functions, compiled straight from its tree.  Run from the
 * repository root (REF = the reference checkout; the binary and the objects go outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/masked_simd
 *   for f in ASM_AVX2/EbBlend_a64_mask_avx2 ASM_AVX2/EbInterPredictionCom_avx2 ASM_SSE2/EbPictureOperators_Intrinsic_SSE2; do
 *     gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 \
 *       -I$C/ASM_SSSE3 -I$C/ASM_SSE4_1 -c $C/$f.c -o /tmp/masked_simd/$(basename $f).o; done
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_masked_compound.c \
 *     /tmp/masked_simd/*.o -o /tmp/gen_golden_masked_compound -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc \
 *     -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_masked_compound tests/golden/masked_compound.bin
 *   /tmp/gen_golden_masked_compound --time   # scripts/masked_compound_perf.py's shapes through the reference's C, one core
 *
 * SIMD: where the CPU has AVX2, every mask and every blend of a block record is made a second time through the reference's
 * _avx2 function and must be equal, and every batch record a second time with the three RTCD pointers bound to the _avx2
 * functions, or the generator stops.  All three AVX2 forms compile stand-alone (the SSE2 file holds the svt_memcpy they
 * call).  The file regenerates byte-identically.
 *
 * Inputs that tests/masked_compound_cases.py rebuilds instead of reading are "drawn" as in gen_golden_compound.c: sample i
 * of stream `seed` is SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) % mod.
 *
 * Records (golden_io format):
 *   wedge     B[100352]  svt_aom_get_contiguous_soft_mask(index, sign, bsize) of the nine sizes with wedges in BlockSize order
 *             (wedge_sizes i32[9][2] {w, h}: 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32, 8x32, 32x8), per size index 0 .. 15,
 *             per index sign 0, 1: w * h bytes with stride w.
 *   nblock, b<i>_par i32[9] {bd, w, h, phase_x, phase_y, kind, content, form, i}: the two CONV_BUF_TYPE blocks c0, c1 [h][w]
 *             are what the reference's jnt_convolve C (form 0 copy, 1 x, 2 y, 3 2d; do_average = 0) gives on the two drawn
 *             sources of gen_golden_compound.c's block records (seed 0x4D43000000000000 + 16 * i + 8 * s; content 0 noise,
 *             1 all zero, 2 all max, 3 max / zero checkerboard with the two sources in opposite phase, 4 max / zero columns
 *             in the sign pattern of the sharp filter's half-sample taps (- + - + + - + -, period 8), the two sources
 *             complementary: no AV1 filter amplifies a checkerboard, so its |c0 - c1| stays at one full-scale step and m at
 *             53 / 54; only overshoot against undershoot reaches the clamp at 64); they are not stored.
 *             b<i>_mask<t> B[h][w] svt_av1_build_compound_diffwtd_mask_d16 of (c0, c1), t 0 DIFFWTD_38, 1 DIFFWTD_38_INV.
 *             b<i>_out<f>: the blend with mask<i & 1> (stride w) for f = subw + 2 * subh of the top-left (w >> subw) x
 *             (h >> subh) corner of c0 and c1 (stride w), present where both dimensions stay >= 4; 8 bits through the lowbd
 *             function, else the highbd one.  b<i>_mm i32[4] {min, max of mask0, min, max of out0}.
 *   nbatch, q<i>_par i32[8] {bd, w, h, n_refs, chroma, border, n_blocks, i}, q<i>_blocks i[n_blocks][16] {x, y, w, h, ref0,
 *             ref1, mv0_x, mv0_y, mv1_x, mv1_y, filter_x, filter_y, comp_type (0 wedge, 1 DIFFWTD), wedge_index, wedge_sign,
 *             mask_type}, q<i>_pred<p> [h][w] the predictor planes (luma only when chroma is 0).  Reference pictures as
 *             gen_golden_compound.c's (seed 0x4D43000000100000 + 256 * i + 4 * r + p), edge-replicated: the record names
 *             `border` samples, the generator replicates 160.
 *   q<i>_kinds i32[52]  how many of the record's blocks / MV components are: wedge of each of the nine sizes (9), of wedge
 *             index 0 .. 15 (16), of sign 0, 1 (2); DIFFWTD of mask type 0, 1 (2), of size 8x8, a 4:1 shape, 64x64, 128x128
 *             (4); a wedge block next to a DIFFWTD block in the list; a DIFFWTD block with ref0 == ref1 and equal MVs (mask 38
 *             everywhere); MV components changed by the clamp at the left / right / top / bottom (4), of odd chroma phase;
 *             filter_x 0 .. 3 (4), filter_y 0 .. 3 (4); the count of blocks (never zero); reserved (3, written as 1).  The
 *             generator stops unless every count is non-zero.
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
#include "EbUtility.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "golden_io.h"

void svt_aom_asm_set_convolve_asm_table(void);
void svt_aom_asm_set_convolve_hbd_asm_table(void);
void svt_av1_init_wedge_masks(void);
/* the reference's AVX2 forms (common_dsp_rtcd.h declares them only under ARCH_X86_64) */
void svt_av1_build_compound_diffwtd_mask_d16_avx2(uint8_t *, DIFFWTD_MASK_TYPE, const CONV_BUF_TYPE *, int, const CONV_BUF_TYPE *, int,
                                                  int, int, ConvolveParams *, int);
void svt_aom_lowbd_blend_a64_d16_mask_avx2(uint8_t *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const CONV_BUF_TYPE *, uint32_t,
                                           const uint8_t *, uint32_t, int, int, int, int, ConvolveParams *);
void svt_aom_highbd_blend_a64_d16_mask_avx2(uint8_t *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const CONV_BUF_TYPE *, uint32_t,
                                            const uint8_t *, uint32_t, int, int, int, int, ConvolveParams *, const int);

typedef void (*MaskFn)(uint8_t *, DIFFWTD_MASK_TYPE, const CONV_BUF_TYPE *, int, const CONV_BUF_TYPE *, int, int, int, ConvolveParams *, int);
typedef void (*Blend8Fn)(uint8_t *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const uint8_t *,
                         uint32_t, int, int, int, int, ConvolveParams *);
typedef void (*Blend16Fn)(uint8_t *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const CONV_BUF_TYPE *, uint32_t, const uint8_t *,
                          uint32_t, int, int, int, int, ConvolveParams *, const int);
static const MaskFn    g_mask[2]    = {svt_av1_build_compound_diffwtd_mask_d16_c, svt_av1_build_compound_diffwtd_mask_d16_avx2};
static const Blend8Fn  g_blend8[2]  = {svt_aom_lowbd_blend_a64_d16_mask_c, svt_aom_lowbd_blend_a64_d16_mask_avx2};
static const Blend16Fn g_blend16[2] = {svt_aom_highbd_blend_a64_d16_mask_c, svt_aom_highbd_blend_a64_d16_mask_avx2};
static void            bind_masked(int pass) {
    svt_av1_build_compound_diffwtd_mask_d16 = g_mask[pass];
    svt_aom_lowbd_blend_a64_d16_mask        = g_blend8[pass];
    svt_aom_highbd_blend_a64_d16_mask       = g_blend16[pass];
}

static int g_simd; /* the CPU has AVX2: the SIMD passes run */

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
static void put_plane(const char *name, int bd, int h, int w, const uint16_t *a, int stride) {
    uint16_t *t  = malloc(sizeof(uint16_t) * w * h);
    uint8_t  *t8 = malloc((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) t[y * w + x] = a[y * stride + x], t8[y * w + x] = (uint8_t)a[y * stride + x];
    put(name, bd > 8 ? 'H' : 'B', 2, h, w, bd > 8 ? (void *)t : (void *)t8);
    free(t), free(t8);
}

static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static PictureControlSet       *g_pcs;
static void                     setup_reference(int w, int h) {
    if (!g_scs) {
        svt_aom_setup_common_rtcd_internal(0);
        svt_aom_setup_rtcd_internal(0);
        svt_aom_asm_set_convolve_asm_table();
        svt_aom_asm_set_convolve_hbd_asm_table();
        bind_masked(0);
        svt_av1_init_wedge_masks();
        svt_aom_build_blk_geom(GEOM_7);
        g_scs = calloc(1, sizeof *g_scs), g_ppcs = calloc(1, sizeof *g_ppcs), g_pcs = calloc(1, sizeof *g_pcs);
        g_pcs->ppcs = g_ppcs, g_pcs->scs = g_scs, g_ppcs->scs = g_scs, g_ppcs->is_not_scaled = 1;
        g_scs->seq_header.sb_size = BLOCK_128X128;
        g_scs->seq_header.order_hint_info.enable_order_hint = 1;
        g_scs->seq_header.order_hint_info.order_hint_bits   = 7;
    }
    svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, w, h, w, h);
}

/* ---- wedge masks ---- */
static const int       g_wsize[9][2] = {{8, 8}, {8, 16}, {16, 8}, {16, 16}, {16, 32}, {32, 16}, {32, 32}, {8, 32}, {32, 8}};
static const BlockSize g_wbsize[9]   = {BLOCK_8X8,   BLOCK_8X16,  BLOCK_16X8, BLOCK_16X16, BLOCK_16X32,
                                        BLOCK_32X16, BLOCK_32X32, BLOCK_8X32, BLOCK_32X8};
static BlockSize       wedge_bsize(int w, int h) {
    for (int k = 0; k < 9; k++)
        if (g_wsize[k][0] == w && g_wsize[k][1] == h) return g_wbsize[k];
    return BLOCK_INVALID;
}
static void gen_wedge(void) {
    uint8_t *all = malloc(100352);
    size_t   n = 0;
    int32_t  sz[9][2];
    setup_reference(64, 64);
    for (int k = 0; k < 9; k++) {
        const int w = g_wsize[k][0], h = g_wsize[k][1];
        sz[k][0] = w, sz[k][1] = h;
        if (block_size_wide[g_wbsize[k]] != w || block_size_high[g_wbsize[k]] != h || svt_aom_get_wedge_bits_lookup(g_wbsize[k]) != 4)
            fprintf(stderr, "wedge size %d\n", k), exit(3);
        for (int i = 0; i < 16; i++)
            for (int s = 0; s < 2; s++) memcpy(all + n, svt_aom_get_contiguous_soft_mask(i, s, g_wbsize[k]), (size_t)w * h), n += (size_t)w * h;
    }
    if (n != 100352) fprintf(stderr, "wedge bytes %zu\n", n), exit(3);
    put("wedge_sizes", 'i', 2, 9, 2, sz);
    put("wedge", 'B', 1, (uint32_t)n, 0, all);
    free(all);
}

/* ---- block records ---- */
static void fill_block(uint16_t *s, int bd, int w, int h, int content, uint64_t seed, int which) {
    const int maxv = (1 << bd) - 1, bw = w + 8, bh = h + 8;
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++)
            s[y * bw + x] = (uint16_t)(content == 0 ? draw(seed, (uint64_t)y * bw + x, maxv + 1)
                                                    : content == 1 ? 0 : content == 2 ? maxv
                                                    : content == 3 ? (((x + y + which) & 1) ? maxv : 0)
                                                                   : ((((0x5A >> (x & 7)) ^ which) & 1) ? maxv : 0));
}
/* the reference's jnt_convolve C with do_average = 0: conv (w x h CONV_BUF_TYPE, stride w) from s */
static void first_pass(int bd, int w, int h, int phx, int phy, int kind, const uint16_t *s, uint16_t *conv) {
    static const AomConvolveFn fn8[4] = {svt_av1_jnt_convolve_2d_copy_c, svt_av1_jnt_convolve_x_c, svt_av1_jnt_convolve_y_c,
                                         svt_av1_jnt_convolve_2d_c};
    static const aom_highbd_convolve_fn_t fn16[4] = {svt_av1_highbd_jnt_convolve_2d_copy_c, svt_av1_highbd_jnt_convolve_x_c,
                                                     svt_av1_highbd_jnt_convolve_y_c, svt_av1_highbd_jnt_convolve_2d_c};
    const int          bw = w + 8, form = (phx ? 1 : 0) | (phy ? 2 : 0);
    InterpFilterParams px, py;
    ConvolveParams     cp = get_conv_params_no_round(0, 0, 0, conv, w, 1, bd);
    av1_get_convolve_filter_params(av1_make_interp_filters((InterpFilter)kind, (InterpFilter)kind), &px, &py, w, h);
    if (bd == 8) {
        uint8_t *s8 = malloc((size_t)bw * (h + 8)), *o8 = malloc((size_t)w * h);
        for (int i = 0; i < bw * (h + 8); i++) s8[i] = (uint8_t)s[i];
        fn8[form](s8 + 3 * bw + 3, bw, o8, w, w, h, &px, &py, phx, phy, &cp);
        free(s8), free(o8);
    } else {
        uint16_t *o = malloc(sizeof(uint16_t) * w * h);
        fn16[form](s + 3 * bw + 3, bw, o, w, w, h, &px, &py, phx, phy, &cp, bd);
        free(o);
    }
}
static void blend(int pass, int bd, uint16_t *out, const uint16_t *c0, const uint16_t *c1, const uint8_t *mask, int stride, int w,
                  int h, int subw, int subh) {
    ConvolveParams cp = get_conv_params_no_round(0, 0, 0, NULL, 0, 1, bd);
    if (bd == 8) {
        uint8_t *o8 = malloc((size_t)w * h);
        g_blend8[pass](o8, w, c0, stride, c1, stride, mask, stride, w, h, subw, subh, &cp);
        for (int i = 0; i < w * h; i++) out[i] = o8[i];
        free(o8);
    } else {
        g_blend16[pass]((uint8_t *)out, w, c0, stride, c1, stride, mask, stride, w, h, subw, subh, &cp, bd);
    }
}
static int gen_blocks(void) {
    /* {w, h, records}: every plane size of a compound block, 4x4 .. 128x128, with every 4:1 shape */
    static const int sizes[22][3] = {{4, 4, 11},   {4, 8, 11},   {8, 4, 11},   {4, 16, 11},  {16, 4, 11},   {8, 8, 11},  {8, 16, 11}, {16, 8, 11},
                                     {8, 32, 3},   {32, 8, 3},   {16, 16, 3},  {16, 32, 2},  {32, 16, 2},   {16, 64, 1}, {64, 16, 1}, {32, 32, 1},
                                     {32, 64, 1},  {64, 32, 1},  {64, 64, 1},  {64, 128, 1}, {128, 64, 1},  {128, 128, 1}};
    static const int bds[3] = {8, 10, 12};
    int              n = 0, seen_m[3][4] = {{0}}, lo[3] = {0}, hi[3] = {0};
    uint16_t        *s = malloc(sizeof(uint16_t) * 136 * 136), *c0 = malloc(sizeof(uint16_t) * 128 * 128), *c1 = malloc(sizeof(uint16_t) * 128 * 128);
    uint16_t        *o = malloc(sizeof(uint16_t) * 128 * 128), *o2 = malloc(sizeof(uint16_t) * 128 * 128);
    uint8_t         *m[2] = {malloc(128 * 128), malloc(128 * 128)}, *m2 = malloc(128 * 128);
    setup_reference(64, 64);
    for (int si = 0; si < 22; si++)
        for (int rep = 0; rep < sizes[si][2]; rep++) {
            const int w = sizes[si][0], h = sizes[si][1];
            /* three bit depths in turn, then the form, then the content: all twenty (form, content) pairs at every bit depth
             * within 60 records.  Content 4 goes with the sharp filter at the half-sample phase, whose signs it follows.
             * 128x128 and 64x128 are 8-bit records, 128x64 a 12-bit one */
            const int form = (n / 3) & 3, content = (n / 12) % 5, kind = content == 4 ? 2 : (n / 3 + n / 12) & 3;
            const int bd = w * h >= 8192 ? (w == 128 && h == 64 ? 12 : 8) : bds[n % 3];
            const int phase = content == 4 ? 8 : n % 5 == 1 ? 15 : n % 7 == 1 ? 3 : 8, phx = (form & 1) ? phase : 0, phy = (form & 2) ? phase : 0;
            ConvolveParams cp = get_conv_params_no_round(0, 0, 0, NULL, 0, 1, bd);
            fill_block(s, bd, w, h, content, 0x4D43000000000000ull + 16 * (uint64_t)n, 0);
            first_pass(bd, w, h, phx, phy, kind, s, c0);
            fill_block(s, bd, w, h, content, 0x4D43000000000000ull + 16 * (uint64_t)n + 8, 1);
            first_pass(bd, w, h, phx, phy, kind, s, c1);
            int32_t mm[4] = {255, 0, 65535, 0}, par[9] = {bd, w, h, phx, phy, kind, content, form, n};
            for (int t = 0; t < 2; t++) {
                g_mask[0](m[t], (DIFFWTD_MASK_TYPE)t, c0, w, c1, w, h, w, &cp, bd);
                if (g_simd) {
                    memset(m2, 0xA5, (size_t)w * h);
                    g_mask[1](m2, (DIFFWTD_MASK_TYPE)t, c0, w, c1, w, h, w, &cp, bd);
                    if (memcmp(m[t], m2, (size_t)w * h)) fprintf(stderr, "avx2 != c: mask of block record %d (%dx%d, %d bits)\n", n, w, h, bd), exit(3);
                }
                put(nm("b%d_mask%d", n, t), 'B', 2, h, w, m[t]);
                for (int i = 0; i < w * h; i++) {
                    const int v = m[t][i];
                    int      *sm = seen_m[bd == 8 ? 0 : bd == 10 ? 1 : 2];
                    sm[0] |= v == 38, sm[1] |= v == 64, sm[2] |= v == 26, sm[3] |= v == 0;
                    if (!t) mm[0] = v < mm[0] ? v : mm[0], mm[1] = v > mm[1] ? v : mm[1];
                }
            }
            for (int f = 0; f < 4; f++) {
                const int subw = f & 1, subh = f >> 1, ow = w >> subw, oh = h >> subh;
                if (ow < 4 || oh < 4) continue;
                blend(0, bd, o, c0, c1, m[n & 1], w, ow, oh, subw, subh);
                if (g_simd) {
                    memset(o2, 0xA5, sizeof(uint16_t) * ow * oh);
                    blend(1, bd, o2, c0, c1, m[n & 1], w, ow, oh, subw, subh);
                    if (memcmp(o, o2, sizeof(uint16_t) * ow * oh))
                        fprintf(stderr, "avx2 != c: blend %d of block record %d (%dx%d, %d bits)\n", f, n, w, h, bd), exit(3);
                }
                put_plane(nm("b%d_out%d", n, f), bd, oh, ow, o, ow);
                if (!f)
                    for (int i = 0; i < w * h; i++) mm[2] = o[i] < mm[2] ? o[i] : mm[2], mm[3] = o[i] > mm[3] ? o[i] : mm[3];
            }
            put(nm("b%d_par", n, 0), 'i', 1, 9, 0, par);
            put(nm("b%d_mm", n, 0), 'i', 1, 4, 0, mm);
            const int k = bd == 8 ? 0 : bd == 10 ? 1 : 2;
            lo[k] |= mm[2] == 0, hi[k] |= mm[3] == (1 << bd) - 1;
            n++;
        }
    for (int k = 0; k < 3; k++) {
        for (int v = 0; v < 4; v++)
            if (!seen_m[k][v]) fprintf(stderr, "%d bits: mask value %d not reached\n", bds[k], v == 0 ? 38 : v == 1 ? 64 : v == 2 ? 26 : 0), exit(3);
        if (!lo[k] || !hi[k]) fprintf(stderr, "%d bits: a clip end not reached\n", bds[k]), exit(3);
    }
    int32_t nn = n;
    put("nblock", 'i', 1, 1, 0, &nn);
    free(s), free(c0), free(c1), free(o), free(o2), free(m[0]), free(m[1]), free(m2);
    return n;
}

/* ---- batch records ---- */
#define PAD 160 /* what the buffers hold */
typedef struct RefPic { /* one padded reference picture: 16-bit samples, and the 8-bit / 2-bit planes the encoder keeps */
    uint16_t *p16[3];
    uint8_t  *p8[3], *p2[3];
    int       stride[3];
} RefPic;
static int pic_value(int bd, uint64_t seed, int pw, int x, int y) {
    const int sc = 1 << (bd - 8);
    return clampi((2 * x + y) * sc / 4 + (int)draw(seed, (uint64_t)y * pw + x, 64 * sc), 0, (1 << bd) - 1);
}
static void ref_alloc(RefPic *r, int bd, int w, int h, uint64_t seed) {
    for (int p = 0; p < 3; p++) {
        const int ss = p > 0, pw = w >> ss, ph = h >> ss, pad = PAD >> ss, st = pw + 2 * pad;
        const size_t n = (size_t)st * (ph + 2 * pad);
        r->stride[p] = st;
        r->p16[p] = malloc(sizeof(uint16_t) * n), r->p8[p] = malloc(n), r->p2[p] = malloc(n);
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) r->p16[p][(y + pad) * st + x + pad] = (uint16_t)pic_value(bd, seed + p, pw, x, y);
        for (int y = -pad; y < ph + pad; y++)
            for (int x = -pad; x < pw + pad; x++) {
                const uint16_t v = r->p16[p][(clampi(y, 0, ph - 1) + pad) * st + clampi(x, 0, pw - 1) + pad];
                const size_t   k = (size_t)(y + pad) * st + x + pad;
                r->p16[p][k] = v;
                if (bd > 8) r->p8[p][k] = (uint8_t)(v >> 2), r->p2[p][k] = (uint8_t)((v & 3) << 6); /* svt_enc_msb_pack2_d's halves */
                else r->p8[p][k] = (uint8_t)v, r->p2[p][k] = 0;
            }
    }
}
static void ref_free(RefPic *r) {
    for (int p = 0; p < 3; p++) free(r->p16[p]), free(r->p8[p]), free(r->p2[p]);
}
static void ref_desc(EbPictureBufferDesc *d, const RefPic *r, int bd, int w, int h) {
    memset(d, 0, sizeof *d);
    d->buffer_y = r->p8[0], d->buffer_cb = r->p8[1], d->buffer_cr = r->p8[2];
    if (bd > 8) d->buffer_bit_inc_y = r->p2[0], d->buffer_bit_inc_cb = r->p2[1], d->buffer_bit_inc_cr = r->p2[2];
    d->org_x = PAD, d->org_y = PAD, d->width = (uint16_t)w, d->height = (uint16_t)h;
    d->stride_y = d->stride_bit_inc_y = (uint16_t)r->stride[0];
    d->stride_cb = d->stride_bit_inc_cb = (uint16_t)r->stride[1];
    d->stride_cr = d->stride_bit_inc_cr = (uint16_t)r->stride[2];
}

typedef struct Block {
    int x, y, w, h, ref0, ref1, mv0[2], mv1[2], fx, fy, type, widx, wsign, mtype;
} Block;
/* a tiling of 256 x 192: {x, y, w, h, comp_type}; every wedge size, DIFFWTD from 8x8 to 128x128 */
static const int g_tiling[][5] = {
    {0, 0, 128, 128, 1},   {128, 0, 64, 64, 1},   {192, 0, 32, 32, 0},   {224, 0, 32, 32, 0},   {192, 32, 32, 16, 0},  {192, 48, 32, 16, 0},
    {224, 32, 16, 32, 0},  {240, 32, 16, 32, 0},  {128, 64, 64, 32, 1},  {128, 96, 64, 16, 1},  {128, 112, 16, 16, 0}, {144, 112, 16, 16, 1},
    {160, 112, 16, 16, 0}, {176, 112, 16, 16, 0}, {192, 64, 16, 64, 1},  {208, 64, 8, 32, 0},   {216, 64, 8, 32, 0},   {208, 96, 8, 32, 1},
    {216, 96, 8, 32, 0},   {224, 64, 32, 8, 0},   {224, 72, 32, 8, 1},   {224, 80, 32, 8, 0},   {224, 88, 32, 8, 0},   {224, 96, 16, 8, 0},
    {240, 96, 16, 8, 1},   {224, 104, 16, 8, 0},  {240, 104, 16, 8, 0},  {224, 112, 8, 16, 0},  {232, 112, 8, 16, 1},  {240, 112, 8, 16, 0},
    {248, 112, 8, 16, 0},  {0, 128, 32, 64, 1},   {32, 128, 64, 32, 1},  {32, 160, 32, 32, 0},  {64, 160, 16, 16, 0},  {64, 176, 16, 16, 1},
    {80, 160, 8, 8, 0},    {88, 160, 8, 8, 1},    {80, 168, 8, 8, 1},    {88, 168, 8, 8, 0},    {80, 176, 16, 16, 0},  {96, 128, 32, 64, 1},
    {128, 128, 128, 64, 1}};
#define N_TILING ((int)(sizeof g_tiling / sizeof g_tiling[0]))
#define SAME_REF_BLOCK 11 /* the DIFFWTD block predicted twice from one reference with one MV */

static int draw_mv(Rng *r, int dim, int k) {
    switch (k % 10) {
    case 0: return 0;
    case 1: return 8 * ((int)rng_below(r, 33) - 16);
    case 5: return (int)rng_below(r, 4001) - 2000;
    case 6: return (rng_below(r, 2) ? 1 : -1) * (dim * 8 + 1000 + (int)rng_below(r, 64));
    case 7: return 2 * ((int)rng_below(r, 9) - 4) + 1;
    case 8: return -(dim * 8 + 1000 + (int)rng_below(r, 64));
    case 9: return dim * 8 + 1000 + (int)rng_below(r, 64);
    default: return (int)rng_below(r, 129) - 64;
    }
}
static void draw_blocks(Block *b, int n, Rng *r, int w, int h, int n_refs) {
    int wedges = 0, diffs = 0;
    for (int k = 0; k < n; k++, b++) {
        b->x = g_tiling[k][0], b->y = g_tiling[k][1], b->w = g_tiling[k][2], b->h = g_tiling[k][3], b->type = g_tiling[k][4];
        b->ref0 = (int)rng_below(r, n_refs), b->ref1 = (int)rng_below(r, n_refs);
        b->mv0[0] = draw_mv(r, w, (int)rng_below(r, 10)), b->mv0[1] = draw_mv(r, h, (int)rng_below(r, 10));
        b->mv1[0] = draw_mv(r, w, (int)rng_below(r, 10)), b->mv1[1] = draw_mv(r, h, (int)rng_below(r, 10));
        if (k == SAME_REF_BLOCK) b->ref1 = b->ref0, b->mv0[0] = b->mv1[0] = 13, b->mv0[1] = b->mv1[1] = -22;
        b->fx = k & 3, b->fy = (k % 3 == 0) ? (k & 3) : (int)rng_below(r, 4);
        b->widx = b->wsign = b->mtype = 0;
        if (b->type == 0)
            b->widx = wedges & 15, b->wsign = ((wedges >> 4) ^ wedges) & 1, wedges++;
        else
            b->mtype = diffs++ & 1;
    }
}
static void count_blocks(int32_t kinds[52], const Block *bl, int n, int w, int h) {
    for (int k = 0; k < n; k++) {
        const Block *b = &bl[k];
        if (b->type == 0) {
            for (int s = 0; s < 9; s++) kinds[s] += g_wsize[s][0] == b->w && g_wsize[s][1] == b->h;
            kinds[9 + b->widx]++, kinds[25 + b->wsign]++;
        } else {
            kinds[27 + b->mtype]++;
            kinds[29] += b->w == 8 && b->h == 8, kinds[30] += b->w == 4 * b->h || b->h == 4 * b->w;
            kinds[31] += b->w == 64 && b->h == 64, kinds[32] += b->w == 128 && b->h == 128;
            kinds[34] += b->ref0 == b->ref1 && b->mv0[0] == b->mv1[0] && b->mv0[1] == b->mv1[1];
        }
        if (k) kinds[33] += b->type != bl[k - 1].type;
        kinds[40 + b->fx]++, kinds[44 + b->fy]++, kinds[48]++;
        for (int m = 0; m < 2; m++) {
            const int *mv = m ? b->mv1 : b->mv0, org[2] = {b->x, b->y}, dim[2] = {w, h}, bs[2] = {b->w, b->h};
            for (int d = 0; d < 2; d++) {
                const int q = (int16_t)(mv[d] * 2), lo = -org[d] * 16 - ((4 + bs[d]) << 4), hi = (dim[d] - bs[d] - org[d]) * 16 + ((4 + bs[d]) << 4) - 16;
                kinds[35 + 2 * d] += q < lo, kinds[36 + 2 * d] += q > hi;
                kinds[39] += (mv[d] & 1);
            }
        }
    }
    kinds[49] = kinds[50] = kinds[51] = 1;
}
static uint32_t find_mds(int w, int h) {
    for (uint32_t k = 0; k < MAX_NUM_BLOCKS_ALLOC; k++) {
        const BlockGeom *g = get_blk_geom_mds(k);
        if (g->bwidth == w && g->bheight == h && g->has_uv) return k;
    }
    fprintf(stderr, "no block geometry of %dx%d\n", w, h), exit(3);
}

/* every block of the list through svt_aom_inter_prediction into the w x h predictor planes (16-bit working samples) */
static void predict_batch(int bd, int w, int h, int chroma, RefPic *refs, Block *blocks, int n, uint16_t *pred[3]) {
    EbPictureBufferDesc rd[3], pd;
    const int           hbd = bd > 8;
    uint8_t            *pb[3];
    for (int r = 0; r < 3; r++) ref_desc(&rd[r], &refs[r], bd, w, h);
    memset(&pd, 0, sizeof pd);
    for (int p = 0; p < 3; p++) pb[p] = calloc((size_t)(w >> (p > 0)) * (h >> (p > 0)), hbd ? 2 : 1);
    pd.buffer_y = pb[0], pd.buffer_cb = pb[1], pd.buffer_cr = pb[2];
    pd.stride_y = (uint16_t)w, pd.stride_cb = pd.stride_cr = (uint16_t)(w / 2), pd.width = (uint16_t)w, pd.height = (uint16_t)h;
    MvReferenceFrame rf[2] = {LAST_FRAME, BWDREF_FRAME};
    const uint8_t    rft = (uint8_t)av1_ref_frame_type(rf);
    g_ppcs->cur_order_hint = 40, g_ppcs->ref_order_hint[LAST_FRAME - 1] = 38, g_ppcs->ref_order_hint[BWDREF_FRAME - 1] = 42;
    for (int k = 0; k < n; k++) {
        Block      *b = &blocks[k];
        BlkStruct   blk;
        MacroBlockD xd;
        MvUnit      mvu;
        InterInterCompoundData comp;
        memset(&blk, 0, sizeof blk), memset(&xd, 0, sizeof xd), memset(&comp, 0, sizeof comp);
        blk.av1xd = &xd, blk.mds_idx = (uint16_t)find_mds(b->w, b->h);
        xd.mb_to_top_edge = -(b->y * 8), xd.mb_to_bottom_edge = (h - b->h - b->y) * 8;
        xd.mb_to_left_edge = -(b->x * 8), xd.mb_to_right_edge = (w - b->w - b->x) * 8;
        mvu.pred_direction = BI_PRED;
        mvu.mv[REF_LIST_0].x = (int16_t)b->mv0[0], mvu.mv[REF_LIST_0].y = (int16_t)b->mv0[1];
        mvu.mv[REF_LIST_1].x = (int16_t)b->mv1[0], mvu.mv[REF_LIST_1].y = (int16_t)b->mv1[1];
        comp.type = b->type ? COMPOUND_DIFFWTD : COMPOUND_WEDGE;
        comp.wedge_index = (uint8_t)b->widx, comp.wedge_sign = (uint8_t)b->wsign, comp.mask_type = (DIFFWTD_MASK_TYPE)b->mtype;
        if (!b->type && wedge_bsize(b->w, b->h) == BLOCK_INVALID) fprintf(stderr, "block %d: no wedges\n", k), exit(3);
        svt_aom_inter_prediction(g_scs, g_pcs, av1_make_interp_filters((InterpFilter)b->fy, (InterpFilter)b->fx), &blk, rft, &mvu, 0,
                                 SIMPLE_TRANSLATION, 0, NULL, 1, &comp, NULL, NULL, NULL, 0, 0, 0, 0, (uint16_t)b->x,
                                 (uint16_t)b->y, (uint8_t)b->w, (uint8_t)b->h, &rd[b->ref0], &rd[b->ref1], &pd, (uint16_t)b->x,
                                 (uint16_t)b->y, chroma ? PICTURE_BUFFER_DESC_FULL_MASK : PICTURE_BUFFER_DESC_LUMA_MASK, (uint8_t)bd, hbd);
    }
    for (int p = 0; p < 3; p++) {
        const size_t cnt = (size_t)(w >> (p > 0)) * (h >> (p > 0));
        for (size_t i = 0; i < cnt; i++) pred[p][i] = hbd ? ((uint16_t *)pb[p])[i] : pb[p][i];
        free(pb[p]);
    }
}

static void gen_batches(void) {
    /* {bd, chroma, inputs of record, declared border}; the third is the first without chroma, the fourth declares less than
     * the replicated 160 */
    static const int cases[4][4] = {{8, 1, 0, 80}, {10, 1, 1, 80}, {8, 0, 0, 80}, {8, 1, 3, 24}};
    const int        w = 256, h = 192, nr = 3, n = N_TILING;
    setup_reference(w, h);
    {
        static uint8_t cover[192][256];
        for (int k = 0; k < n; k++) {
            const int *t = g_tiling[k];
            for (int y = t[1]; y < t[1] + t[3]; y++)
                for (int x = t[0]; x < t[0] + t[2]; x++) cover[y][x]++;
        }
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (cover[y][x] != 1) fprintf(stderr, "tiling: (%d, %d) covered %d times\n", x, y, cover[y][x]), exit(3);
    }
    for (int i = 0; i < 4; i++) {
        const int bd = cases[i][0], chroma = cases[i][1], src = cases[i][2], border = cases[i][3];
        Rng       r = {0x4D43000000080000ull + src};
        Block     blocks[N_TILING];
        RefPic    refs[3];
        uint16_t *pred[3], *again[3];
        int32_t   kinds[52] = {0}, par[8] = {bd, w, h, nr, chroma, border, n, src};
        draw_blocks(blocks, n, &r, w, h, nr);
        for (int k = 0; k < nr; k++) ref_alloc(&refs[k], bd, w, h, 0x4D43000000100000ull + 256 * (uint64_t)src + 4 * k);
        for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2), again[p] = calloc((size_t)w * h, 2);
        predict_batch(bd, w, h, chroma, refs, blocks, n, pred);
        if (g_simd) {
            bind_masked(1);
            predict_batch(bd, w, h, chroma, refs, blocks, n, again);
            bind_masked(0);
            for (int p = 0; p < 3; p++)
                if (memcmp(again[p], pred[p], (size_t)w * h * 2)) fprintf(stderr, "avx2 != c: batch record %d plane %d\n", i, p), exit(3);
        }
        count_blocks(kinds, blocks, n, w, h);
        for (int k = 0; k < 52; k++)
            if (!kinds[k]) fprintf(stderr, "batch record %d: nothing of kind %d\n", i, k), exit(3);
        int32_t *rec = malloc(sizeof(int32_t) * n * 16);
        for (int k = 0; k < n; k++) {
            const Block *b = &blocks[k];
            const int32_t v[16] = {b->x, b->y, b->w, b->h, b->ref0, b->ref1, b->mv0[0], b->mv0[1], b->mv1[0], b->mv1[1], b->fx, b->fy,
                                   b->type, b->widx, b->wsign, b->mtype};
            memcpy(rec + 16 * k, v, sizeof v);
        }
        put(nm("q%d_par", i, 0), 'i', 1, 8, 0, par);
        put(nm("q%d_blocks", i, 0), 'i', 2, n, 16, rec);
        put(nm("q%d_kinds", i, 0), 'i', 1, 52, 0, kinds);
        for (int p = 0; p < (chroma ? 3 : 1); p++) put_plane(nm("q%d_pred%d", i, p), bd, h >> (p > 0), w >> (p > 0), pred[p], w >> (p > 0));
        free(rec);
        for (int k = 0; k < nr; k++) ref_free(&refs[k]);
        for (int p = 0; p < 3; p++) free(pred[p]), free(again[p]);
    }
    int32_t nb = 4;
    put("nbatch", 'i', 1, 1, 0, &nb);
}

/* scripts/masked_compound_perf.py's workloads through the reference's C on one core: gen_golden_compound.c's tiling (all 17
 * sizes, 23 blocks per 256 x 192) repeated over the picture, once all-wedge (blocks larger than 32 split into 32 x 32) and
 * once all-DIFFWTD */
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
    for (int k = 0; k < 2; k++)
        for (int type = 0; type < 2; type++) {
            const int bd = shapes[k][0], w = shapes[k][1], h = shapes[k][2], cols = w / 256, rows = h / 192;
            Rng       r = {0x4D43000000300000ull};
            Block    *blocks = calloc((size_t)cols * rows * 23 * 16, sizeof(Block));
            RefPic    refs[3];
            uint16_t *pred[3];
            int       n = 0;
            setup_reference(w, h);
            for (int q = 0; q < cols * rows; q++)
                for (int j = 0; j < 23; j++) {
                    const int *t = g_perf_tiling[j], cw = !type && t[2] > 32 ? 32 : t[2], ch = !type && t[3] > 32 ? 32 : t[3];
                    for (int oy = 0; oy < t[3]; oy += ch)
                        for (int ox = 0; ox < t[2]; ox += cw) {
                            /* a wedge block has one of the nine sizes: 32 x 8 pieces of 64 x 16 and the like are fine, a
                             * 32 x 32 piece of anything larger too */
                            Block *b = &blocks[n];
                            b->x = t[0] + ox + (q % cols) * 256, b->y = t[1] + oy + (q / cols) * 192, b->w = cw, b->h = ch;
                            if (!type && wedge_bsize(cw, ch) == BLOCK_INVALID) b->w = b->h = cw < ch ? cw : ch; /* never: all pieces have wedges */
                            b->ref0 = (int)rng_below(&r, 3), b->ref1 = (int)rng_below(&r, 3);
                            for (int d = 0; d < 2; d++) b->mv0[d] = (int)rng_below(&r, 1025) - 512, b->mv1[d] = (int)rng_below(&r, 1025) - 512;
                            b->fx = j & 3, b->fy = (j >> 1) & 3, b->type = type, b->widx = n & 15, b->wsign = (n >> 4) & 1, b->mtype = n & 1;
                            n++;
                        }
                }
            for (int q = 0; q < 3; q++) ref_alloc(&refs[q], bd, w, h, 0x4D43000000400000ull + 4 * q);
            for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2);
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                const double t0 = now_ms();
                predict_batch(bd, w, h, 1, refs, blocks, n, pred);
                const double t1 = now_ms();
                if (t1 - t0 < best) best = t1 - t0;
            }
            printf("{\"workload\": \"%dx%d %d-bit, %d %s blocks over %dx%d\", \"predict_c_ms\": %.2f, \"reps\": 3}\n", w, h, bd, n,
                   type ? "DIFFWTD" : "wedge", cols * 256, rows * 192, best);
            for (int q = 0; q < 3; q++) ref_free(&refs[q]);
            for (int p = 0; p < 3; p++) free(pred[p]);
            free(blocks);
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
    gen_wedge();
    const int nb = gen_blocks();
    gen_batches();
    golden_close(&g);
    fprintf(stderr, "288 wedge masks, %d block records, 4 batch records; %s\n", nb,
            g_simd ? "every mask, blend and batch record equal through the _avx2 functions" : "no AVX2 on this host: the _c functions only");
    return 0;
}
