/*
 * gen_golden_compound.c — writes tests/golden/compound.bin: the reference's compound (two-reference) prediction: the
 * eight svt_av1_(highbd_)jnt_convolve_{2d,x,y,2d_copy}_c functions (EbInterPrediction.c:503-677, :861-1040), the weight
 * selection of svt_av1_dist_wtd_comp_weight_assign (:276-318) and svt_aom_inter_prediction with is_compound = 1
 * (EbEncInterPrediction.c:4070) on deterministic inputs (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration) and the reference's AVX2 jnt_convolve sources, compiled straight from its tree.  Run from the
 * repository root (REF = the reference checkout; the binary and the objects go outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/compound_simd
 *   for f in ASM_AVX2/jnt_convolve_avx2 ASM_AVX2/jnt_convolve_2d_avx2 ASM_AVX2/highbd_jnt_convolve_avx2; do
 *     gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 \
 *       -I$C/ASM_SSSE3 -I$C/ASM_SSE4_1 -c $C/$f.c -o /tmp/compound_simd/$(basename $f).o; done
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_compound.c \
 *     /tmp/compound_simd/*.o -o /tmp/gen_golden_compound -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc \
 *     -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_compound tests/golden/compound.bin
 *   /tmp/gen_golden_compound --time   # scripts/compound_perf.py's shapes through the reference's C and AVX2, one core
 *
 * SIMD: where the CPU has AVX2, every block record is made a second time through the reference's _avx2 function and must
 * be equal (first-pass CONV_BUF_TYPE block and pixels), and every batch record a second time with the eight RTCD pointers
 * bound to the _avx2 functions (svt_aom_convolve[][][] / svt_aom_convolveHbd[][][] rebuilt from them), or the generator
 * stops.  The file regenerates byte-identically.
 *
 * Inputs that tests/compound_cases.py rebuilds instead of reading are "drawn": sample i of stream `seed` is
 * SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) % mod, golden_io.h's generator started at seed + i * the constant.
 *
 * Records (golden_io format):
 *   weights   i[34][34][2][2]  {fwd_offset, bck_offset} for (d0, d1, order_idx), the distances handed to
 *             svt_av1_dist_wtd_comp_weight_assign as order hints (it clamps them to MAX_FRAME_DISTANCE itself).
 *   nblock, b<i>_par i32[12] {bd, w, h, phase_x, phase_y, kind, content, form, i, dist_wtd, fwd_offset, bck_offset},
 *             b<i>_conv H[h][w] the CONV_BUF_TYPE block after the first call (do_average = 0) on source 0, b<i>_out [h][w]
 *             the pixels after the second call (do_average = 1) on source 1, b<i>_mm i32[2] {min, max} of them.  kind 0
 *             EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR for both directions, the parameters through
 *             av1_get_convolve_filter_params (w <= 4 / h <= 4 take the 4-tap tables); form 0 copy, 1 x, 2 y, 3 2d, chosen
 *             by the phases being non-zero as svt_inter_predictor does; rounds from get_conv_params_no_round(is_compound
 *             = 1).  Source s is a drawn (h + 8) x (w + 8) buffer (seed 0x4A4E000000000000 + 16 * i + 8 * s) with the block
 *             at (3, 3): content 0 noise, 1 all zero, 2 all max, 3 max / zero checkerboard ((x + y + s) & 1).
 *   nbatch, q<i>_par i32[8] {bd, w, h, n_refs, chroma, border, n_blocks, i}, q<i>_blocks i[n_blocks][15] {x, y, w, h, ref0,
 *             ref1, mv0_x, mv0_y, mv1_x, mv1_y, filter_x, filter_y, dist_wtd, fwd_offset, bck_offset}, q<i>_pred<p> [h][w]
 *             the predictor planes (luma only when chroma is 0).  Reference picture r, plane p is drawn over the picture
 *             (seed 0x4A4E000000100000 + 256 * i + 4 * r + p, value clamp((2 * x + y) * sc / 4 + draw % (64 * sc))) with
 *             edge-replicated borders; the record names 80 luma / 40 chroma samples, the generator replicates 160 / 80 so
 *             that the reference's own reads (a 128x128 block reaches 135 samples out, and its 10-bit path packs 8 more)
 *             stay inside its buffers: on replicated borders the samples are the same.
 *   q<i>_kinds i32[27]      how many of the record's blocks / MV components are: COMPOUND_AVERAGE, COMPOUND_DISTWTD; with
 *             filter_x 0 .. 3 (4 counts), filter_y 0 .. 3 (4), filter_x != filter_y, ref0 == ref1; MVs zero, integer; MV
 *             components of luma phase 1 .. 7 eighths (7), changed by the clamp at the left / right / top / bottom (4),
 *             wholly outside the picture after it, of odd chroma phase.  The generator stops unless every count is non-zero.
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
/* the reference's AVX2 forms (common_dsp_rtcd.h declares them only under ARCH_X86_64) */
#define SIMD_8(n) \
    void n(const uint8_t *, int32_t, uint8_t *, int32_t, int32_t, int32_t, InterpFilterParams *, InterpFilterParams *, \
           const int32_t, const int32_t, ConvolveParams *)
#define SIMD_16(n)                                                                                       \
    void n(const uint16_t *, int32_t, uint16_t *, int32_t, int32_t, int32_t, const InterpFilterParams *, \
           const InterpFilterParams *, const int32_t, const int32_t, ConvolveParams *, int32_t)
SIMD_8(svt_av1_jnt_convolve_2d_copy_avx2);
SIMD_8(svt_av1_jnt_convolve_x_avx2);
SIMD_8(svt_av1_jnt_convolve_y_avx2);
SIMD_8(svt_av1_jnt_convolve_2d_avx2);
SIMD_16(svt_av1_highbd_jnt_convolve_2d_copy_avx2);
SIMD_16(svt_av1_highbd_jnt_convolve_x_avx2);
SIMD_16(svt_av1_highbd_jnt_convolve_y_avx2);
SIMD_16(svt_av1_highbd_jnt_convolve_2d_avx2);
/* form 0 copy, 1 x, 2 y, 3 2d; pass 0 the _c functions, 1 _avx2 */
static const AomConvolveFn g_fn8[2][4] = {
    {svt_av1_jnt_convolve_2d_copy_c, svt_av1_jnt_convolve_x_c, svt_av1_jnt_convolve_y_c, svt_av1_jnt_convolve_2d_c},
    {svt_av1_jnt_convolve_2d_copy_avx2, svt_av1_jnt_convolve_x_avx2, svt_av1_jnt_convolve_y_avx2, svt_av1_jnt_convolve_2d_avx2}};
static const aom_highbd_convolve_fn_t g_fn16[2][4] = {
    {svt_av1_highbd_jnt_convolve_2d_copy_c, svt_av1_highbd_jnt_convolve_x_c, svt_av1_highbd_jnt_convolve_y_c,
     svt_av1_highbd_jnt_convolve_2d_c},
    {svt_av1_highbd_jnt_convolve_2d_copy_avx2, svt_av1_highbd_jnt_convolve_x_avx2, svt_av1_highbd_jnt_convolve_y_avx2,
     svt_av1_highbd_jnt_convolve_2d_avx2}};
static void bind_convolve(int pass) {
    svt_av1_jnt_convolve_2d_copy = g_fn8[pass][0], svt_av1_jnt_convolve_x = g_fn8[pass][1];
    svt_av1_jnt_convolve_y = g_fn8[pass][2], svt_av1_jnt_convolve_2d = g_fn8[pass][3];
    svt_av1_highbd_jnt_convolve_2d_copy = g_fn16[pass][0], svt_av1_highbd_jnt_convolve_x = g_fn16[pass][1];
    svt_av1_highbd_jnt_convolve_y = g_fn16[pass][2], svt_av1_highbd_jnt_convolve_2d = g_fn16[pass][3];
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
static const char *nm(const char *fmt, int i, int a) {
    static char s[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(s[k], sizeof s[k], fmt, i, a);
    return s[k];
}
static void put(const char *name, char dt, int ndim, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, const void *data) {
    uint32_t dims[4] = {d0, d1, d2, d3};
    golden_put(g_file, name, dt, ndim, dims, data);
}
static void put_plane(const char *name, int bd, int h, int w, const uint16_t *a, int stride) {
    uint16_t *t  = malloc(sizeof(uint16_t) * w * h);
    uint8_t  *t8 = malloc((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) t[y * w + x] = a[y * stride + x], t8[y * w + x] = (uint8_t)a[y * stride + x];
    put(name, bd > 8 ? 'H' : 'B', 2, h, w, 0, 0, bd > 8 ? (void *)t : (void *)t8);
    free(t), free(t8);
}

static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static PictureControlSet       *g_pcs;
static void                     setup_reference(int w, int h) {
    if (!g_scs) {
        svt_aom_setup_common_rtcd_internal(0);
        svt_aom_setup_rtcd_internal(0);
        bind_convolve(0);
        svt_aom_build_blk_geom(GEOM_7);
        g_scs = calloc(1, sizeof *g_scs), g_ppcs = calloc(1, sizeof *g_ppcs), g_pcs = calloc(1, sizeof *g_pcs);
        g_pcs->ppcs = g_ppcs, g_pcs->scs = g_scs, g_ppcs->scs = g_scs, g_ppcs->is_not_scaled = 1;
        g_scs->seq_header.sb_size = BLOCK_128X128;
        g_scs->seq_header.order_hint_info.enable_order_hint = 1;
        g_scs->seq_header.order_hint_info.order_hint_bits   = 7;
    }
    svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, w, h, w, h);
}

/* ---- weights ---- */
static void gen_weights(void) {
    static int32_t t[34][34][2][2];
    setup_reference(64, 64);
    for (int d0 = 0; d0 < 34; d0++)
        for (int d1 = 0; d1 < 34; d1++)
            for (int o = 0; o < 2; o++) {
                int fwd = -1, bck = -1, use = -1;
                /* cur 40, the backward reference d1 before it, the forward one d0 after it (7 order-hint bits: +-64) */
                svt_av1_dist_wtd_comp_weight_assign(&g_scs->seq_header, 40, 40 - d1, 40 + d0, 0, o, &fwd, &bck, &use, 1);
                if (use != 1) fprintf(stderr, "weights: not assigned\n"), exit(3);
                t[d0][d1][o][0] = fwd, t[d0][d1][o][1] = bck;
            }
    put("weights", 'i', 4, 34, 34, 2, 2, t);
}

/* the nine combine modes of a block record: plain average, then the eight pairs of quant_dist_lookup_table */
static const int g_modes[9][3] = {{0, 0, 0}, {1, 9, 7}, {1, 11, 5}, {1, 12, 4}, {1, 13, 3}, {1, 7, 9}, {1, 5, 11}, {1, 4, 12}, {1, 3, 13}};

/* ---- block records ---- */
static void fill_block(uint16_t *s, int bd, int w, int h, int content, uint64_t seed, int which) {
    const int maxv = (1 << bd) - 1, bw = w + 8, bh = h + 8;
    for (int y = 0; y < bh; y++)
        for (int x = 0; x < bw; x++)
            s[y * bw + x] = (uint16_t)(content == 0 ? draw(seed, (uint64_t)y * bw + x, maxv + 1)
                                                    : content == 1 ? 0 : content == 2 ? maxv : ((x + y + which) & 1) ? maxv : 0);
}
/* the two calls of one block: conv (w x h CONV_BUF_TYPE) from s0, out from s1 */
static void run_block(int pass, int bd, int w, int h, int phx, int phy, int kind, const int *mode, const uint16_t *s0,
                      const uint16_t *s1, uint16_t *conv, uint16_t *out) {
    const int          bw = w + 8, form = (phx ? 1 : 0) | (phy ? 2 : 0);
    InterpFilterParams px, py;
    ConvolveParams     cp = get_conv_params_no_round(0, 0, 0, conv, w, 1, bd);
    av1_get_convolve_filter_params(av1_make_interp_filters((InterpFilter)kind, (InterpFilter)kind), &px, &py, w, h);
    uint8_t *s8 = malloc((size_t)bw * (h + 8)), *o8 = malloc((size_t)w * h);
    for (int call = 0; call < 2; call++) {
        const uint16_t *s = call ? s1 : s0;
        if (call) cp.do_average = 1, cp.use_jnt_comp_avg = cp.use_dist_wtd_comp_avg = mode[0], cp.fwd_offset = mode[1], cp.bck_offset = mode[2];
        if (bd == 8) {
            for (int i = 0; i < bw * (h + 8); i++) s8[i] = (uint8_t)s[i];
            memset(o8, 0, (size_t)w * h);
            g_fn8[pass][form](s8 + 3 * bw + 3, bw, o8, w, w, h, &px, &py, phx, phy, &cp);
            for (int i = 0; i < w * h; i++) out[i] = o8[i];
        } else {
            g_fn16[pass][form](s + 3 * bw + 3, bw, out, w, w, h, &px, &py, phx, phy, &cp, bd);
        }
    }
    free(s8), free(o8);
}
static int gen_blocks(void) {
    /* the 17 compound block sizes and what their 4:2:0 chroma adds (4x4, 4x8, 8x4, 4x16, 16x4) */
    static const int sizes[22][2] = {{4, 4}, {4, 8}, {8, 4}, {4, 16}, {16, 4}, {8, 8}, {8, 16}, {16, 8}, {8, 32}, {32, 8}, {16, 16},
                                     {16, 32}, {32, 16}, {16, 64}, {64, 16}, {32, 32}, {32, 64}, {64, 32}, {64, 64}, {64, 128},
                                     {128, 64}, {128, 128}};
    static const int ph[3] = {0, 5, 15}, bds[3] = {8, 10, 12};
    int              n = 0, seen[2][4] = {{0}}, lo[3] = {0}, hi[3] = {0}, big = 0;
    uint16_t        *s0 = malloc(sizeof(uint16_t) * 136 * 136), *s1 = malloc(sizeof(uint16_t) * 136 * 136);
    uint16_t        *c = malloc(sizeof(uint16_t) * 128 * 128), *o = malloc(sizeof(uint16_t) * 128 * 128);
    uint16_t        *c2 = malloc(sizeof(uint16_t) * 128 * 128), *o2 = malloc(sizeof(uint16_t) * 128 * 128);
    for (int si = 0; si < 22; si++)
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const int w = sizes[si][0], h = sizes[si][1];
                /* below 128 samples all nine phase pairs; below 1024 one record per form; from 1024 up (nine sizes) one
                 * record each, the form rotating over them */
                if (w * h >= 128 && (a == 1 || b == 1)) continue;
                if (w * h >= 1024 && (((a ? 1 : 0) | (b ? 2 : 0)) != (big & 3))) continue;
                const int phx = ph[a], phy = ph[b], form = (phx ? 1 : 0) | (phy ? 2 : 0);
                const int bd = bds[n % 3], kind = (n / 3) & 3, content = (1 + seen[bd > 8][form]) & 3;
                const int *mode = g_modes[n % 9 == 0 ? (n / 9) % 9 : n % 9]; /* every mode at every bit depth and kind in turn */
                fill_block(s0, bd, w, h, content, 0x4A4E000000000000ull + 16 * (uint64_t)n, 0);
                fill_block(s1, bd, w, h, content, 0x4A4E000000000000ull + 16 * (uint64_t)n + 8, 1);
                run_block(0, bd, w, h, phx, phy, kind, mode, s0, s1, c, o);
                if (g_simd) {
                    memset(c2, 0xA5, sizeof(uint16_t) * w * h), memset(o2, 0xA5, sizeof(uint16_t) * w * h);
                    run_block(1, bd, w, h, phx, phy, kind, mode, s0, s1, c2, o2);
                    if (memcmp(c, c2, sizeof(uint16_t) * w * h) || memcmp(o, o2, sizeof(uint16_t) * w * h))
                        fprintf(stderr, "avx2 != c: block record %d (%dx%d, %d bits, form %d)\n", n, w, h, bd, form), exit(3);
                }
                int32_t mm[2] = {65535, 0}, par[12] = {bd, w, h, phx, phy, kind, content, form, n, mode[0], mode[1], mode[2]};
                for (int i = 0; i < w * h; i++) mm[0] = o[i] < mm[0] ? o[i] : mm[0], mm[1] = o[i] > mm[1] ? o[i] : mm[1];
                put(nm("b%d_par", n, 0), 'i', 1, 12, 0, 0, 0, par);
                put(nm("b%d_conv", n, 0), 'H', 2, h, w, 0, 0, c);
                put_plane(nm("b%d_out", n, 0), bd, h, w, o, w);
                put(nm("b%d_mm", n, 0), 'i', 1, 2, 0, 0, 0, mm);
                seen[bd > 8][form]++, lo[n % 3] |= mm[0] == 0, hi[n % 3] |= mm[1] == (1 << bd) - 1;
                if (w * h >= 1024) big++;
                n++;
            }
    for (int k = 0; k < 8; k++)
        if (!seen[k >> 2][k & 3]) fprintf(stderr, "function %d: not hit\n", k), exit(3);
    for (int k = 0; k < 3; k++)
        if (!lo[k] || !hi[k]) fprintf(stderr, "%d bits: a clip end not reached\n", bds[k]), exit(3);
    int32_t nn = n;
    put("nblock", 'i', 1, 1, 0, 0, 0, &nn);
    free(s0), free(s1), free(c), free(o), free(c2), free(o2);
    return n;
}

/* ---- batch records ---- */
#define BORDER 80 /* what the record names */
#define PAD 160   /* what the buffers hold */
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
    int x, y, w, h, ref0, ref1, mv0[2], mv1[2], fx, fy, dist, fwd, bck, d0, d1;
} Block;
/* a tiling of 256 x 192 with all 17 sizes */
static const int g_tiling[][4] = {
    {0, 0, 128, 128},   {128, 0, 128, 64},  {128, 64, 64, 128}, {192, 64, 64, 64},  {192, 128, 64, 32},  {192, 160, 32, 32},
    {224, 160, 32, 16}, {224, 176, 16, 16}, {240, 176, 8, 16},  {248, 176, 8, 8},   {248, 184, 8, 8},    {0, 128, 32, 64},
    {32, 128, 64, 32},  {32, 160, 64, 16},  {32, 176, 32, 8},   {32, 184, 32, 8},   {64, 176, 16, 16},   {80, 176, 16, 8},
    {80, 184, 16, 8},   {96, 128, 16, 64},  {112, 128, 16, 32}, {112, 160, 8, 32},  {120, 160, 8, 32}};
#define N_TILING ((int)(sizeof g_tiling / sizeof g_tiling[0]))

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
    for (int k = 0; k < n; k++, b++) {
        b->x = g_tiling[k][0], b->y = g_tiling[k][1], b->w = g_tiling[k][2], b->h = g_tiling[k][3];
        b->ref0 = (int)rng_below(r, n_refs), b->ref1 = k % 5 == 0 ? b->ref0 : (int)rng_below(r, n_refs);
        const int both_zero = k % 11 == 3, both_int = k % 11 == 4;
        b->mv0[0] = both_zero ? 0 : both_int ? 16 : draw_mv(r, w, (int)rng_below(r, 10)), b->mv0[1] = both_zero ? 0 : both_int ? -8 : draw_mv(r, h, (int)rng_below(r, 10));
        b->mv1[0] = both_zero ? 0 : both_int ? -24 : draw_mv(r, w, (int)rng_below(r, 10)), b->mv1[1] = both_zero ? 0 : both_int ? 0 : draw_mv(r, h, (int)rng_below(r, 10));
        /* every eighth-sample phase, on MVs too small for the clamp to act */
        if (!both_zero && !both_int && k % 3 == 1) b->mv0[0] = 8 * ((int)rng_below(r, 9) - 4) + (k / 3) % 7 + 1;
        if (!both_zero && !both_int && k % 3 == 2) b->mv1[1] = 8 * ((int)rng_below(r, 9) - 4) + (k / 3 + 1) % 7 + 1;
        b->fx = k & 3, b->fy = (k % 3 == 0) ? (k & 3) : (int)rng_below(r, 4);
        b->dist = k & 1, b->d0 = 1 + (int)rng_below(r, 9), b->d1 = 1 + (int)rng_below(r, 9);
        b->fwd = b->bck = 0;
    }
}
static void count_block(int32_t kinds[27], const Block *b, int w, int h) {
    kinds[b->dist ? 1 : 0]++, kinds[2 + b->fx]++, kinds[6 + b->fy]++, kinds[10] += b->fx != b->fy, kinds[11] += b->ref0 == b->ref1;
    for (int m = 0; m < 2; m++) {
        const int *mv = m ? b->mv1 : b->mv0, org[2] = {b->x, b->y}, dim[2] = {w, h}, bs[2] = {b->w, b->h};
        kinds[12] += !mv[0] && !mv[1];
        kinds[13] += (mv[0] || mv[1]) && !(mv[0] & 7) && !(mv[1] & 7);
        for (int d = 0; d < 2; d++) {
            const int q = (int16_t)(mv[d] * 2), lo = -org[d] * 16 - ((4 + bs[d]) << 4), hi = (dim[d] - bs[d] - org[d]) * 16 + ((4 + bs[d]) << 4) - 16;
            const int c = clampi(q, lo, hi), pos = org[d] + (c >> 4);
            if (c & 15) kinds[14 + ((c & 15) >> 1) - 1]++;
            kinds[21 + 2 * d] += q < lo, kinds[22 + 2 * d] += q > hi;
            kinds[25] += pos + bs[d] <= 0 || pos >= dim[d];
            kinds[26] += (mv[d] & 1);
        }
    }
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
        comp.type = b->dist ? COMPOUND_DISTWTD : COMPOUND_AVERAGE;
        /* the weights come from the frame distances: rf[0] (LAST) d1 before the current frame, rf[1] (BWDREF) d0 after it */
        g_ppcs->cur_order_hint = 40, g_ppcs->ref_order_hint[LAST_FRAME - 1] = 40 - b->d1, g_ppcs->ref_order_hint[BWDREF_FRAME - 1] = 40 + b->d0;
        if (b->dist) {
            int use;
            svt_av1_dist_wtd_comp_weight_assign(&g_scs->seq_header, 40, 40 - b->d1, 40 + b->d0, 0, 0, &b->fwd, &b->bck, &use, 1);
        }
        svt_aom_inter_prediction(g_scs, g_pcs, av1_make_interp_filters((InterpFilter)b->fy, (InterpFilter)b->fx), &blk, rft, &mvu, 0,
                                 SIMPLE_TRANSLATION, 0, NULL, b->dist ? 0 : 1, &comp, NULL, NULL, NULL, 0, 0, 0, 0, (uint16_t)b->x,
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
    static const int cases[3][2] = {{8, 1}, {10, 1}, {8, 0}}; /* {bd, chroma}; the third is the first without chroma */
    const int        w = 256, h = 192, nr = 3, n = N_TILING;
    setup_reference(w, h);
    /* the tiling covers the picture once, with all 17 sizes */
    {
        static uint8_t cover[192][256];
        int            sizes = 0, seen[8][8] = {{0}};
        for (int k = 0; k < n; k++) {
            const int *t = g_tiling[k];
            for (int y = t[1]; y < t[1] + t[3]; y++)
                for (int x = t[0]; x < t[0] + t[2]; x++) cover[y][x]++;
            int wl = 0, hl = 0;
            while ((1 << wl) < t[2]) wl++;
            while ((1 << hl) < t[3]) hl++;
            sizes += !seen[wl][hl]++;
        }
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                if (cover[y][x] != 1) fprintf(stderr, "tiling: (%d, %d) covered %d times\n", x, y, cover[y][x]), exit(3);
        if (sizes != 17) fprintf(stderr, "tiling: %d sizes\n", sizes), exit(3);
    }
    for (int i = 0; i < 3; i++) {
        const int bd = cases[i][0], chroma = cases[i][1], src = i == 2 ? 0 : i; /* inputs of record `src` */
        Rng       r = {0x4A4E000000080000ull + src};
        Block     blocks[N_TILING];
        RefPic    refs[3];
        uint16_t *pred[3], *again[3];
        int32_t   kinds[27] = {0}, par[8] = {bd, w, h, nr, chroma, BORDER, n, src};
        draw_blocks(blocks, n, &r, w, h, nr);
        for (int k = 0; k < nr; k++) ref_alloc(&refs[k], bd, w, h, 0x4A4E000000100000ull + 256 * (uint64_t)src + 4 * k);
        for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2), again[p] = calloc((size_t)w * h, 2);
        predict_batch(bd, w, h, chroma, refs, blocks, n, pred);
        if (g_simd) {
            bind_convolve(1);
            predict_batch(bd, w, h, chroma, refs, blocks, n, again);
            bind_convolve(0);
            for (int p = 0; p < 3; p++)
                if (memcmp(again[p], pred[p], (size_t)w * h * 2)) fprintf(stderr, "avx2 != c: batch record %d plane %d\n", i, p), exit(3);
        }
        for (int k = 0; k < n; k++) count_block(kinds, &blocks[k], w, h);
        for (int k = 0; k < 27; k++)
            if (!kinds[k]) fprintf(stderr, "batch record %d: nothing of kind %d\n", i, k), exit(3);
        int32_t *rec = malloc(sizeof(int32_t) * n * 15);
        for (int k = 0; k < n; k++) {
            const Block *b = &blocks[k];
            const int32_t v[15] = {b->x, b->y, b->w, b->h, b->ref0, b->ref1, b->mv0[0], b->mv0[1], b->mv1[0], b->mv1[1], b->fx, b->fy,
                                   b->dist, b->fwd, b->bck};
            memcpy(rec + 15 * k, v, sizeof v);
        }
        put(nm("q%d_par", i, 0), 'i', 1, 8, 0, 0, 0, par);
        put(nm("q%d_blocks", i, 0), 'i', 2, n, 15, 0, 0, rec);
        put(nm("q%d_kinds", i, 0), 'i', 1, 27, 0, 0, 0, kinds);
        for (int p = 0; p < (chroma ? 3 : 1); p++) put_plane(nm("q%d_pred%d", i, p), bd, h >> (p > 0), w >> (p > 0), pred[p], w >> (p > 0));
        free(rec);
        for (int k = 0; k < nr; k++) ref_free(&refs[k]);
        for (int p = 0; p < 3; p++) free(pred[p]), free(again[p]);
    }
    int32_t nb = 3;
    put("nbatch", 'i', 1, 1, 0, 0, 0, &nb);
}

/* scripts/compound_perf.py's workloads through the reference's C and AVX2 on one core: the tiling repeated over the picture */
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static void time_reference(void) {
    static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
    for (int k = 0; k < 2; k++) {
        const int bd = shapes[k][0], w = shapes[k][1], h = shapes[k][2], cols = w / 256, rows = h / 192, n = cols * rows * N_TILING;
        Rng       r = {0x4A4E000000300000ull};
        Block    *blocks = calloc(n, sizeof(Block)), one[N_TILING];
        RefPic    refs[3];
        uint16_t *pred[3];
        setup_reference(w, h);
        for (int q = 0; q < cols * rows; q++) {
            draw_blocks(one, N_TILING, &r, w, h, 3);
            for (int j = 0; j < N_TILING; j++) {
                one[j].x += (q % cols) * 256, one[j].y += (q / cols) * 192;
                for (int d = 0; d < 2; d++) one[j].mv0[d] = clampi(one[j].mv0[d], -512, 512), one[j].mv1[d] = clampi(one[j].mv1[d], -512, 512);
                blocks[q * N_TILING + j] = one[j];
            }
        }
        for (int q = 0; q < 3; q++) ref_alloc(&refs[q], bd, w, h, 0x4A4E000000400000ull + 4 * q);
        for (int p = 0; p < 3; p++) pred[p] = calloc((size_t)w * h, 2);
        double ms[2] = {0, 0};
        for (int pass = 0; pass <= g_simd; pass++) {
            bind_convolve(pass);
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                const double t0 = now_ms();
                predict_batch(bd, w, h, 1, refs, blocks, n, pred);
                const double t1 = now_ms();
                if (t1 - t0 < best) best = t1 - t0;
            }
            ms[pass] = best;
        }
        bind_convolve(0);
        printf("{\"workload\": \"%dx%d %d-bit, %d blocks over %dx%d\", \"predict_c_ms\": %.2f, \"predict_avx2_ms\": %.2f, \"reps\": 3}\n",
               w, h, bd, n, cols * 256, rows * 192, ms[0], ms[1]);
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
    gen_weights();
    const int nb = gen_blocks();
    gen_batches();
    golden_close(&g);
    fprintf(stderr, "2312 weight pairs, %d block records, 3 batch records; %s\n", nb,
            g_simd ? "every block and batch record equal through the _avx2 functions" : "no AVX2 on this host: the _c functions only");
    return 0;
}
