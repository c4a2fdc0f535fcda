/*
 * gen_golden_interintra.c — writes tests/golden/interintra.bin: the reference's inter-intra prediction,
 * svt_aom_inter_prediction with is_interintra_used = 1 (EbEncInterPrediction.c:4070, :4487, inter_intra_prediction :2548), on
 * deterministic pictures (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration).  Run from the repository root (REF = the reference checkout; the binary goes outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/ii_simd
 *   gcc -O2 -msse4.1 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 -I$C/ASM_SSSE3 \
 *     -I$C/ASM_SSE4_1 -c $C/ASM_SSE4_1/EbBlend_a64_mask_sse4.c -o /tmp/ii_simd/EbBlend_a64_mask_sse4.o
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_interintra.c /tmp/ii_simd/*.o \
 *     -o /tmp/gen_golden_interintra -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_interintra tests/golden/interintra.bin
 *   /tmp/gen_golden_interintra --time   # scripts/interintra_perf.py's lists through the reference's C, one core
 *
 * A record is a picture of at most 96 x 64: a set of blocks ("cells") of the seven inter-intra sizes at multiples of 8, each with
 * a reference, an MV, a dual filter, an inter-intra mode, a wedge flag and index, and its availability: whether there is a row
 * above / a column left (xd's up / left flags: off at the picture's edge, and drawn off elsewhere as at a tile's edge) and by how
 * many luma samples the block hangs over the right / bottom edge (mb_to_right_edge / mb_to_bottom_edge below zero, for cells at that
 * edge), which shortens n_top_px / n_left_px.  The harness builds the three NeighborArrayUnits from drawn "recon" samples and the
 * MacroBlockD; every cell is predicted through svt_aom_inter_prediction into the record's predictor picture.
 *
 * The edge preparation is NOT restated: while a block is predicted the entries of svt_aom_eb_pred / svt_aom_dc_pred and their
 * highbd tables are recorders that note which predictor build_intra_predictors chose and the prepared above / left arrays it
 * hands over, then call the table's own (_c) function.  A plane for which no predictor ran took the early constant fill.
 *
 * Pictures are drawn as gen_golden_obmc_pred.c's (seed 0x4949000000100000 + 256 * i + 4 * r + p), or constant / alternating by
 * `content`; tests/interintra_cases.py rebuilds them.  The neighbour arrays: top[x] of plane p is draw(seed_n + p, x, 1 << bd), left[y]
 * draw(seed_n + 4 + p, y, 1 << bd), seed_n = 0x4949000000200000 + 256 * i; for content 1 / 2 all zero / all max.  The source luma of
 * the search records is draw(0x4949000000300000 + 256 * i, y * w + x, 1 << bd) (content 1, 3: zero; 2: max).
 *
 * Records (golden_io format):
 *   nrec; r<i>_par i32[9] {bd, w, h, n_refs, chroma, border, n_blocks, content, i};
 *   r<i>_blocks i32[n_blocks][22]: {x, y, w, h, ref, filter_x, filter_y, mv_x, mv_y, mode, use_wedge, wedge_index, n_top (luma),
 *   n_top (chroma), n_left (luma), n_left (chroma), edge_offset, kind Y, kind Cb, kind Cr, hang_x, hang_y}; kind 0 dc, 1 dc_top, 2
 *   dc_left, 3 dc_128, 4 v, 5 h, 6 smooth, 7 the early fill (chroma kinds -1 without chroma);
 *   r<i>_edges [n_edges] the edge pool as svtgpu_interintra_predict_batch takes it (raw neighbour samples; entries beyond a count
 *   hold what the arrays held); r<i>_prep [n_edges] in the same layout the prepared arrays the recorders saw (0 where a predictor
 *   does not read: left for v, above for h, both for the fill);
 *   r<i>_pred<p> [h][w] the predictor planes (0 where no block writes; luma only when chroma is 0);
 *   r<i>_sse i64[n_blocks][4]: the search records: per mode the luma predictor of the block with use_wedge = 0 (through
 *   svt_aom_combine_interintra(_highbd)) against the source by svt_aom_sse_c / svt_aom_highbd_sse_c.
 *   b<k>_par i32[8] {hbd, w, h, subw, subh, bd, k, extremes}, b<k>_out: the blend records (inputs by seed 0x4949000000400000 + 16 * k);
 *   i<k>_par i32[6] {hbd, w, h, kind, bd, k}, i<k>_out: the intra records (above / left by seed 0x4949000000500000 + 16 * k).
 *   counts i32[NCOUNT]: how often each case below occurred over the file; the generator stops unless every one is non-zero.
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
#include "EbIntraPrediction.h"
#include "EbModeDecisionProcess.h"
#include "EbNeighborArrays.h"
#include "EbReferenceObject.h"
#include "EbUtility.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "golden_io.h"

#define BORDER 80
#define PAD 160
#define NBCOLS 22

enum { /* counts[] */
    C_SIZE8 = 0,    /* 7: size k at 8 bits */
    C_SIZE10 = 7,   /* 7: at 10 bits */
    C_MODE = 14,    /* 4 */
    C_WEDGE = 18,   /* 2: smooth, wedge */
    C_WINDEX = 20,  /* 16 */
    C_AVAIL = 36,   /* 9: (n_top class) * 3 + (n_left class) of luma, class 0 none, 1 partial, 2 full */
    C_HANG = 45,    /* 2: a partial count from mb_to_right_edge / mb_to_bottom_edge */
    C_COL0 = 47, C_ROW0 = 48, C_RIGHT = 49, C_BOTTOM = 50,
    C_FORM = 51,    /* 4: the own pass's convolve form: copy, x, y, 2-D */
    C_CONTENT = 55, /* 3: all zero, all max, checkerboard */
    C_LO = 58, C_HI = 59,     /* a blended sample reaching 0 / the maximum */
    C_DC_UP = 60, C_DC_DOWN = 61, /* a DC sum (dc of both sides) whose remainder rounds up / down */
    C_NOCHROMA = 62, C_CHROMA = 63,
    C_KIND = 64,    /* 8: the recorded luma kind, 7 the fill */
    NCOUNT = 72
};
static int32_t g_counts[NCOUNT];
static double  g_ms_pred;
static double  now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static uint32_t draw(uint64_t seed, uint64_t i, uint32_t mod) {
    Rng r = {seed + i * 0x9E3779B97F4A7C15ull};
    return (uint32_t)(rng_next(&r) % mod);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
static const int g_sizes[7][2] = {{8, 8}, {8, 16}, {16, 8}, {16, 16}, {16, 32}, {32, 16}, {32, 32}};
static int       size_index(int w, int h) {
    for (int k = 0; k < 7; k++)
        if (g_sizes[k][0] == w && g_sizes[k][1] == h) return k;
    return -1;
}
static const int g_psizes[10][2] = {{4, 4}, {4, 8}, {8, 4}, {8, 8}, {8, 16}, {16, 8}, {16, 16}, {16, 32}, {32, 16}, {32, 32}};

void svt_aom_asm_set_convolve_asm_table(void);
void svt_aom_asm_set_convolve_hbd_asm_table(void);
void svt_aom_init_intra_predictors_internal(void);

static GoldenFile *g_file;
static const char *nm(const char *fmt, int i, int a) {
    static char s[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(s[k], sizeof s[k], fmt, i, a);
    return s[k];
}
static void put(const char *name, char dt, int ndim, uint32_t d0, uint32_t d1, const void *data) {
    if (!g_file) return; /* --time: nothing is written */
    uint32_t dims[2] = {d0, d1};
    golden_put(g_file, name, dt, ndim, dims, data);
}

/* ---- the recorders ---- */
static IntraPredFn     g_eb[INTRA_MODES][TX_SIZES_ALL], g_dc[2][2][TX_SIZES_ALL];
static IntraHighPredFn g_ebh[INTRA_MODES][TX_SIZES_ALL], g_dch[2][2][TX_SIZES_ALL];
static struct {
    int      w, h, calls, kind[3];
    uint16_t above[3][32], left[3][32];
} g_rec;
static TxSize tx_of(int w, int h) {
    for (int t = 0; t < TX_SIZES_ALL; t++)
        if (tx_size_wide[t] == w && tx_size_high[t] == h) return (TxSize)t;
    fprintf(stderr, "no tx size %dx%d\n", w, h), exit(3);
}
/* the plane of this call: the reference predicts Y, Cb, Cr in order, one predictor call each (none for the early fill, which
 * note_fill() accounts for from the outside) */
static int g_plane;
static void note(int kind, const void *above, const void *left, int hbd, int *w, int *h) {
    const int p = g_plane;
    *w = g_rec.w >> (p > 0), *h = g_rec.h >> (p > 0);
    g_rec.kind[p] = kind, g_rec.calls++;
    const int need_above = kind != 5, need_left = kind != 4; /* h does not read above, v not left */
    for (int i = 0; i < *w; i++) g_rec.above[p][i] = need_above ? (hbd ? ((const uint16_t *)above)[i] : ((const uint8_t *)above)[i]) : 0;
    for (int i = 0; i < *h; i++) g_rec.left[p][i] = need_left ? (hbd ? ((const uint16_t *)left)[i] : ((const uint8_t *)left)[i]) : 0;
}
#define RECORDER(kind, name, lookup8, lookup16)                                                          \
    static void rec8_##name(uint8_t *dst, ptrdiff_t stride, const uint8_t *above, const uint8_t *left) { \
        int w, h;                                                                                        \
        note(kind, above, left, 0, &w, &h);                                                              \
        const TxSize t = tx_of(w, h);                                                                    \
        (lookup8)(dst, stride, above, left);                                                             \
    }                                                                                                    \
    static void rec16_##name(uint16_t *dst, ptrdiff_t stride, const uint16_t *above, const uint16_t *left, int32_t bd) { \
        int w, h;                                                                                        \
        note(kind, above, left, 1, &w, &h);                                                              \
        const TxSize t = tx_of(w, h);                                                                    \
        (lookup16)(dst, stride, above, left, bd);                                                        \
    }
RECORDER(0, dc, g_dc[1][1][t], g_dch[1][1][t])
RECORDER(1, dc_top, g_dc[0][1][t], g_dch[0][1][t])
RECORDER(2, dc_left, g_dc[1][0][t], g_dch[1][0][t])
RECORDER(3, dc_128, g_dc[0][0][t], g_dch[0][0][t])
RECORDER(4, v, g_eb[V_PRED][t], g_ebh[V_PRED][t])
RECORDER(5, h, g_eb[H_PRED][t], g_ebh[H_PRED][t])
RECORDER(6, smooth, g_eb[SMOOTH_PRED][t], g_ebh[SMOOTH_PRED][t])
static void bind_recorders(int on) {
    for (int t = 0; t < TX_SIZES_ALL; t++) {
        svt_aom_dc_pred[1][1][t] = on ? rec8_dc : g_dc[1][1][t], svt_aom_dc_pred_high[1][1][t] = on ? rec16_dc : g_dch[1][1][t];
        svt_aom_dc_pred[0][1][t] = on ? rec8_dc_top : g_dc[0][1][t], svt_aom_dc_pred_high[0][1][t] = on ? rec16_dc_top : g_dch[0][1][t];
        svt_aom_dc_pred[1][0][t] = on ? rec8_dc_left : g_dc[1][0][t], svt_aom_dc_pred_high[1][0][t] = on ? rec16_dc_left : g_dch[1][0][t];
        svt_aom_dc_pred[0][0][t] = on ? rec8_dc_128 : g_dc[0][0][t], svt_aom_dc_pred_high[0][0][t] = on ? rec16_dc_128 : g_dch[0][0][t];
        svt_aom_eb_pred[V_PRED][t] = on ? rec8_v : g_eb[V_PRED][t], svt_aom_pred_high[V_PRED][t] = on ? rec16_v : g_ebh[V_PRED][t];
        svt_aom_eb_pred[H_PRED][t] = on ? rec8_h : g_eb[H_PRED][t], svt_aom_pred_high[H_PRED][t] = on ? rec16_h : g_ebh[H_PRED][t];
        svt_aom_eb_pred[SMOOTH_PRED][t] = on ? rec8_smooth : g_eb[SMOOTH_PRED][t];
        svt_aom_pred_high[SMOOTH_PRED][t] = on ? rec16_smooth : g_ebh[SMOOTH_PRED][t];
    }
}
/* the blends run once per plane, after the plane's intra prediction: they advance the plane the next predictor call is for */
static void blend8(uint8_t *dst, uint32_t ds, const uint8_t *s0, uint32_t s0s, const uint8_t *s1, uint32_t s1s, const uint8_t *m,
                   uint32_t ms, int w, int h, int sx, int sy) {
    g_plane++, svt_aom_blend_a64_mask_c(dst, ds, s0, s0s, s1, s1s, m, ms, w, h, sx, sy);
}
static void blend16(uint8_t *dst, uint32_t ds, const uint8_t *s0, uint32_t s0s, const uint8_t *s1, uint32_t s1s, const uint8_t *m,
                    uint32_t ms, int w, int h, int sx, int sy, int bd) {
    g_plane++, svt_aom_highbd_blend_a64_mask_c(dst, ds, s0, s0s, s1, s1s, m, ms, w, h, sx, sy, bd);
}

/* ---- the reference's structures ---- */
static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static PictureControlSet       *g_pcs;
static Av1Common               *g_cm;
static EbPictureBufferDesc      g_enh;
static EbObjectWrapper          g_wrap[3];
static EbReferenceObject        g_refobj[3];
static const MvReferenceFrame   g_frame_of[3] = {LAST_FRAME, LAST2_FRAME, BWDREF_FRAME};

static void setup_reference(int w, int h) {
    if (!g_scs) {
        svt_aom_setup_common_rtcd_internal(0);
        svt_aom_setup_rtcd_internal(0);
        svt_aom_asm_set_convolve_asm_table();
        svt_aom_asm_set_convolve_hbd_asm_table();
        svt_aom_init_intra_predictors_internal();
        svt_av1_init_wedge_masks();
        svt_aom_build_blk_geom(GEOM_7);
        memcpy(g_eb, svt_aom_eb_pred, sizeof g_eb), memcpy(g_dc, svt_aom_dc_pred, sizeof g_dc);
        memcpy(g_ebh, svt_aom_pred_high, sizeof g_ebh), memcpy(g_dch, svt_aom_dc_pred_high, sizeof g_dch);
        g_scs = calloc(1, sizeof *g_scs), g_ppcs = calloc(1, sizeof *g_ppcs), g_pcs = calloc(1, sizeof *g_pcs);
        g_cm = calloc(1, sizeof *g_cm);
        g_pcs->ppcs = g_ppcs, g_pcs->scs = g_scs, g_ppcs->scs = g_scs, g_ppcs->is_not_scaled = 1;
        g_ppcs->av1_cm = g_cm, g_ppcs->enhanced_pic = &g_enh;
        g_scs->seq_header.sb_size = BLOCK_128X128, g_scs->sb_size = 128;
        for (int r = 0; r < 3; r++) g_wrap[r].object_ptr = &g_refobj[r];
        g_pcs->ref_pic_ptr_array[0][0] = &g_wrap[0], g_pcs->ref_pic_ptr_array[0][1] = &g_wrap[1];
        g_pcs->ref_pic_ptr_array[1][0] = &g_wrap[2];
    }
    svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, w, h, w, h);
    g_cm->mi_cols = w / 4, g_cm->mi_rows = h / 4, g_cm->subsampling_x = g_cm->subsampling_y = 1;
    memset(&g_enh, 0, sizeof g_enh);
    g_enh.width = (uint16_t)w, g_enh.height = (uint16_t)h;
}

typedef struct RefPic {
    uint16_t *p16[3];
    uint8_t  *p8[3], *p2[3];
    int       stride[3];
} RefPic;
static int pic_value(int bd, uint64_t seed, int pw, int x, int y, int content, int r) {
    const int sc = 1 << (bd - 8), maxv = (1 << bd) - 1;
    if (content == 1) return 0;
    if (content == 2) return maxv;
    if (content == 3) return ((x + y + r) & 1) ? maxv : 0;
    return clampi((2 * x + y) * sc / 4 + (int)draw(seed, (uint64_t)y * pw + x, 64 * sc), 0, maxv);
}
static void ref_alloc(RefPic *r, int bd, int w, int h, uint64_t seed, int content, int ri) {
    for (int p = 0; p < 3; p++) {
        const int    ss = p > 0, pw = w >> ss, ph = h >> ss, pad = PAD >> ss, st = pw + 2 * pad;
        const size_t n = (size_t)st * (ph + 2 * pad);
        r->stride[p] = st;
        r->p16[p] = malloc(sizeof(uint16_t) * n), r->p8[p] = malloc(n), r->p2[p] = malloc(n);
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) r->p16[p][(y + pad) * st + x + pad] = (uint16_t)pic_value(bd, seed + p, pw, x, y, content, ri);
        for (int y = -pad; y < ph + pad; y++)
            for (int x = -pad; x < pw + pad; x++) {
                const uint16_t v = r->p16[p][(clampi(y, 0, ph - 1) + pad) * st + clampi(x, 0, pw - 1) + pad];
                const size_t   k = (size_t)(y + pad) * st + x + pad;
                r->p16[p][k] = v;
                if (bd > 8) r->p8[p][k] = (uint8_t)(v >> 2), r->p2[p][k] = (uint8_t)((v & 3) << 6);
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
    d->bit_depth = bd > 8 ? EB_TEN_BIT : EB_EIGHT_BIT;
    d->stride_y = d->stride_bit_inc_y = (uint16_t)r->stride[0];
    d->stride_cb = d->stride_bit_inc_cb = (uint16_t)r->stride[1];
    d->stride_cr = d->stride_bit_inc_cr = (uint16_t)r->stride[2];
}

/* ---- scenes ---- */
typedef struct Cell {
    int x, y, w, h, ref, mv[2], fx, fy, mode, wedge, windex, up, left, hang_x, hang_y;
} Cell;
#define MAXC 64
typedef struct Scene {
    int  w, h, n;
    Cell c[MAXC];
} Scene;
static uint32_t find_mds(int w, int h) {
    for (uint32_t k = 0; k < MAX_NUM_BLOCKS_ALLOC; k++) {
        const BlockGeom *g = get_blk_geom_mds(k);
        if (g->bwidth == w && g->bheight == h && g->has_uv) return k;
    }
    fprintf(stderr, "no block geometry of %dx%d\n", w, h), exit(3);
}
/* the 96 x 64 tiling: all seven sizes, every edge and corner */
static const int g_tiling[18][4] = {{0, 0, 32, 32},  {32, 0, 32, 16},  {32, 16, 16, 16}, {48, 16, 16, 8},  {48, 24, 8, 8},  {56, 24, 8, 8},
                                    {64, 0, 16, 32}, {80, 0, 8, 16},   {88, 0, 8, 16},   {80, 16, 16, 16}, {0, 32, 16, 32}, {16, 32, 32, 32},
                                    {48, 32, 32, 16}, {48, 48, 16, 16}, {64, 48, 16, 8},  {64, 56, 8, 8},   {72, 56, 8, 8},  {80, 32, 16, 32}};
/* MVs in 1/8 sample: small with every phase, integer, zero, large enough for a clamp on either side */
static int draw_mv(Rng *r, int dim) {
    switch (rng_below(r, 8)) {
    case 0: return 0;
    case 1: return 8 * ((int)rng_below(r, 17) - 8);
    case 2: return dim * 8 + 400 + (int)rng_below(r, 64);
    case 3: return -(dim * 8 + 400 + (int)rng_below(r, 64));
    case 4: return 2 * ((int)rng_below(r, 9) - 4) + 1;
    default: return (int)rng_below(r, 161) - 80;
    }
}
static void add_cell(Scene *s, int x, int y, int w, int h) {
    if (s->n >= MAXC) fprintf(stderr, "scene: too many cells\n"), exit(3);
    Cell *c = &s->c[s->n++];
    memset(c, 0, sizeof *c);
    c->x = x, c->y = y, c->w = w, c->h = h, c->up = y > 0, c->left = x > 0;
}
static void draw_cells(Scene *s, Rng *r) {
    for (int k = 0; k < s->n; k++) {
        Cell *c = &s->c[k];
        c->ref = (int)rng_below(r, 3), c->fx = (int)rng_below(r, 4), c->fy = (int)rng_below(r, 4);
        c->mv[0] = draw_mv(r, s->w), c->mv[1] = draw_mv(r, s->h);
        c->mode = (int)rng_below(r, 4), c->wedge = (int)rng_below(r, 2), c->windex = (int)rng_below(r, 16);
        c->up = c->y > 0 && rng_below(r, 4) != 0, c->left = c->x > 0 && rng_below(r, 4) != 0; /* off: as at a tile's edge */
        /* a cell at the right / bottom edge may hang over it by half its side; its MV stays small: the library clamps MVs
         * against the picture it was given, in which the block lies whole (include/svtgpu.h) */
        c->hang_x = (c->x + c->w == s->w && rng_below(r, 2)) ? c->w / 2 : 0;
        c->hang_y = (c->y + c->h == s->h && rng_below(r, 2)) ? c->h / 2 : 0;
        if (c->hang_x) c->mv[0] = (int)rng_below(r, 33) - 16;
        if (c->hang_y) c->mv[1] = (int)rng_below(r, 33) - 16;
    }
}

/* the neighbour arrays of one plane: top[x], left[y] drawn; the arrays are longer than the picture, as the reference copies two
 * block lengths */
typedef struct Neigh {
    NeighborArrayUnit u;
    uint16_t          top[256], left[256];
    uint8_t           top8[512], left8[512], tl[2048];
} Neigh;
static void neigh_fill(Neigh *n, int p, int bd, uint64_t seed, int content, int pic_h) {
    const int maxv = (1 << bd) - 1;
    memset(n, 0, sizeof *n);
    for (int i = 0; i < 256; i++) {
        n->top[i] = (uint16_t)(content == 1 ? 0 : content == 2 ? maxv : draw(seed + p, i, maxv + 1));
        n->left[i] = (uint16_t)(content == 1 ? 0 : content == 2 ? maxv : draw(seed + 4 + p, i, maxv + 1));
        n->top8[i] = (uint8_t)n->top[i], n->left8[i] = (uint8_t)n->left[i];
    }
    n->u.top_array = bd > 8 ? (uint8_t *)n->top : n->top8, n->u.left_array = bd > 8 ? (uint8_t *)n->left : n->left8;
    n->u.top_left_array = n->tl, n->u.max_pic_h = (uint32_t)pic_h;
}

/* one prediction of cell c into pd (component mask by `chroma`), mode / wedge as given; the recorders are bound */
static void predict(const Scene *s, const Cell *c, int bd, int chroma, int mode, int wedge, EbPictureBufferDesc *rd, EbPictureBufferDesc *pd,
                    Neigh *nb) {
    const int   w = s->w, h = s->h, hbd = bd > 8;
    BlkStruct   blk;
    MacroBlockD xd;
    MvUnit      mvu;
    memset(&blk, 0, sizeof blk), memset(&xd, 0, sizeof xd), memset(&mvu, 0, sizeof mvu);
    blk.av1xd = &xd, blk.mds_idx = (uint16_t)find_mds(c->w, c->h);
    xd.mb_to_top_edge = -(c->y * 8), xd.mb_to_bottom_edge = (h - c->h - c->y) * 8 - c->hang_y * 8;
    xd.mb_to_left_edge = -(c->x * 8), xd.mb_to_right_edge = (w - c->w - c->x) * 8 - c->hang_x * 8;
    xd.n4_w = (uint8_t)(c->w / 4), xd.n4_h = (uint8_t)(c->h / 4), xd.n8_w = (uint8_t)(c->w / 8), xd.n8_h = (uint8_t)(c->h / 8);
    xd.up_available = xd.chroma_up_available = c->up, xd.left_available = xd.chroma_left_available = c->left;
    xd.mi_row = c->y / 4, xd.mi_col = c->x / 4;
    xd.tile.mi_col_end = w / 4, xd.tile.mi_row_end = h / 4;
    mvu.pred_direction = UNI_PRED_LIST_0;
    mvu.mv[REF_LIST_0].x = (int16_t)c->mv[0], mvu.mv[REF_LIST_0].y = (int16_t)c->mv[1];
    MvReferenceFrame rf[2] = {g_frame_of[c->ref], NONE_FRAME};
    memset(&g_rec, 0, sizeof g_rec);
    g_rec.w = c->w, g_rec.h = c->h, g_rec.kind[0] = g_rec.kind[1] = g_rec.kind[2] = 7, g_plane = 0;
    if (!chroma) g_rec.kind[1] = g_rec.kind[2] = -1;
    const double t0 = now_ms();
    svt_aom_inter_prediction(g_scs, g_pcs, av1_make_interp_filters((InterpFilter)c->fy, (InterpFilter)c->fx), &blk,
                             (uint8_t)av1_ref_frame_type(rf), &mvu, 0, SIMPLE_TRANSLATION, 0, NULL, 1, NULL, &nb[0].u, &nb[1].u, &nb[2].u, 1,
                             (InterIntraMode)mode, (uint8_t)wedge, c->windex, (uint16_t)c->x, (uint16_t)c->y, (uint8_t)c->w, (uint8_t)c->h,
                             &rd[c->ref], NULL, pd, (uint16_t)c->x, (uint16_t)c->y,
                             chroma ? PICTURE_BUFFER_DESC_FULL_MASK : PICTURE_BUFFER_DESC_LUMA_MASK, (uint8_t)bd, hbd);
    g_ms_pred += now_ms() - t0;
    if (g_plane != (chroma ? 3 : 1)) fprintf(stderr, "recorder: %d blends\n", g_plane), exit(3);
}

static int edge_len(const Cell *c, int chroma) { return (c->w + c->h) * (chroma ? 2 : 1); }
static int avail_class(int n, int side) { return n == 0 ? 0 : n < side ? 1 : 2; }

static void gen_record(int idx, const Scene *s, int bd, int chroma, int content) {
    const int w = s->w, h = s->h, hbd = bd > 8, maxv = (1 << bd) - 1;
    setup_reference(w, h);
    RefPic              refs[3];
    EbPictureBufferDesc rd[3], pd;
    for (int r = 0; r < 3; r++) {
        ref_alloc(&refs[r], bd, w, h, 0x4949000000100000ull + 256 * (uint64_t)idx + 4 * r, content, r);
        ref_desc(&rd[r], &refs[r], bd, w, h);
        g_refobj[r].reference_picture = &rd[r];
    }
    static Neigh nb[3];
    for (int p = 0; p < 3; p++) neigh_fill(&nb[p], p, bd, 0x4949000000200000ull + 256 * (uint64_t)idx, content, h >> (p > 0));
    uint8_t *pb[3], *tb;
    memset(&pd, 0, sizeof pd);
    for (int p = 0; p < 3; p++) pb[p] = calloc((size_t)(w >> (p > 0)) * (h >> (p > 0)), hbd ? 2 : 1);
    pd.buffer_y = pb[0], pd.buffer_cb = pb[1], pd.buffer_cr = pb[2];
    pd.stride_y = (uint16_t)w, pd.stride_cb = pd.stride_cr = (uint16_t)(w / 2), pd.width = (uint16_t)w, pd.height = (uint16_t)h;
    pd.bit_depth = bd > 8 ? EB_TEN_BIT : EB_EIGHT_BIT;
    /* the search records' own predictor picture, and the source */
    EbPictureBufferDesc td = pd;
    tb = calloc((size_t)w * h, hbd ? 2 : 1), td.buffer_y = tb;
    uint16_t *src16 = malloc(sizeof(uint16_t) * w * h);
    uint8_t  *src8 = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++) {
        src16[i] = (uint16_t)(content == 2 ? maxv : (content == 1 || content == 3) ? 0 : draw(0x4949000000300000ull + 256 * (uint64_t)idx, i, maxv + 1));
        src8[i] = (uint8_t)src16[i];
    }
    svt_aom_blend_a64_mask = blend8, svt_aom_highbd_blend_a64_mask = blend16;
    bind_recorders(1);

    int n_edges = 0;
    for (int k = 0; k < s->n; k++) n_edges += edge_len(&s->c[k], chroma);
    int32_t  *rec = calloc((size_t)s->n * NBCOLS, sizeof(int32_t));
    uint16_t *edges = calloc(n_edges + 1, sizeof(uint16_t)), *prep = calloc(n_edges + 1, sizeof(uint16_t));
    int64_t  *sse = calloc((size_t)s->n * 4, sizeof(int64_t));
    int       eo = 0;
    for (int k = 0; k < s->n; k++) {
        const Cell *c = &s->c[k];
        const int   si = size_index(c->w, c->h);
        if (si < 0 || (c->x & 7) || (c->y & 7)) fprintf(stderr, "record %d: cell %d\n", idx, k), exit(3);
        predict(s, c, bd, chroma, c->mode, c->wedge, rd, &pd, nb);
        int32_t *o = rec + NBCOLS * k;
        /* n_top_px / n_left_px as svt_av1_predict_intra_block computes them from the availability this harness set */
        int n_top[2], n_left[2];
        for (int q = 0; q < 2; q++) {
            const int pw = c->w >> q, ph = c->h >> q, xr = (-(c->hang_x * 8)) >> (3 + q), yd = (-(c->hang_y * 8)) >> (3 + q);
            n_top[q] = c->up ? (pw < xr + pw ? pw : xr + pw) : 0, n_left[q] = c->left ? (ph < yd + ph ? ph : yd + ph) : 0;
        }
        const int32_t head[NBCOLS] = {c->x, c->y, c->w, c->h, c->ref, c->fx, c->fy, c->mv[0], c->mv[1], c->mode, c->wedge, c->windex,
                                      n_top[0], n_top[1], n_left[0], n_left[1], eo, g_rec.kind[0], g_rec.kind[1], g_rec.kind[2],
                                      c->hang_x, c->hang_y};
        memcpy(o, head, sizeof head);
        int e = eo;
        for (int p = 0; p < (chroma ? 3 : 1); p++) {
            const int ss = p > 0, pw = c->w >> ss, ph = c->h >> ss;
            for (int i = 0; i < pw; i++) edges[e + i] = nb[p].top[(c->x >> ss) + i], prep[e + i] = g_rec.above[p][i];
            for (int i = 0; i < ph; i++) edges[e + pw + i] = nb[p].left[(c->y >> ss) + i], prep[e + pw + i] = g_rec.left[p][i];
            e += pw + ph;
        }
        eo = e;
        /* the counters */
        g_counts[(hbd ? C_SIZE10 : C_SIZE8) + si]++, g_counts[C_MODE + c->mode]++, g_counts[C_WEDGE + c->wedge]++;
        if (c->wedge) g_counts[C_WINDEX + c->windex]++;
        g_counts[C_AVAIL + 3 * avail_class(n_top[0], c->w) + avail_class(n_left[0], c->h)]++;
        g_counts[C_HANG] += c->hang_x && c->up, g_counts[C_HANG + 1] += c->hang_y && c->left;
        g_counts[C_COL0] += c->x == 0, g_counts[C_ROW0] += c->y == 0, g_counts[C_RIGHT] += c->x + c->w == w, g_counts[C_BOTTOM] += c->y + c->h == h;
        {   /* the own pass's form, from the clamped MV's phases (clamp_mv_to_umv_border_sb; luma: 1/16 sample, phases even) */
            int ph2[2];
            for (int d = 0; d < 2; d++) {
                const int b = d ? c->h : c->w, org = d ? c->y : c->x, dim = (d ? h - c->hang_y : w - c->hang_x), spel = (4 + b) << 4;
                const int q = (int16_t)(c->mv[d] * 2), lo = -(org * 8) * 2 - spel, hi = ((dim - b - org) * 8) * 2 + spel - 16;
                ph2[d] = (int16_t)(q < lo ? lo : q > hi ? hi : q) & 15;
            }
            g_counts[C_FORM + (ph2[0] ? 1 : 0) + (ph2[1] ? 2 : 0)]++;
        }
        g_counts[C_CONTENT + 0] += content == 1, g_counts[C_CONTENT + 1] += content == 2, g_counts[C_CONTENT + 2] += content == 3;
        g_counts[chroma ? C_CHROMA : C_NOCHROMA]++, g_counts[C_KIND + g_rec.kind[0]]++;
        if (content == 0 || content == 3) {
            int lo = 65535, hi = 0;
            for (int y = c->y; y < c->y + c->h; y++)
                for (int x = c->x; x < c->x + c->w; x++) {
                    const int v = hbd ? ((uint16_t *)pb[0])[y * w + x] : pb[0][y * w + x];
                    lo = v < lo ? v : lo, hi = v > hi ? v : hi;
                }
            g_counts[C_LO] += lo == 0, g_counts[C_HI] += hi == maxv;
        }
        if (g_rec.kind[0] == 0) {
            int sum = 0;
            for (int i = 0; i < c->w; i++) sum += g_rec.above[0][i];
            for (int i = 0; i < c->h; i++) sum += g_rec.left[0][i];
            const int rem = sum % (c->w + c->h);
            g_counts[C_DC_UP] += 2 * rem >= c->w + c->h, g_counts[C_DC_DOWN] += rem && 2 * rem < c->w + c->h;
        }
        /* the search record: four modes, the smooth blend, luma, against the source */
        for (int m = 0; m < 4 && g_file; m++) { /* --time: the predictions only */
            predict(s, c, bd, 0, m, 0, rd, &td, nb);
            const size_t off = (size_t)c->y * w + c->x;
            sse[4 * k + m] = hbd ? svt_aom_highbd_sse_c((uint8_t *)(src16 + off), w, (uint8_t *)((uint16_t *)tb + off), w, c->w, c->h)
                                 : svt_aom_sse_c(src8 + off, w, tb + off, w, c->w, c->h);
        }
    }
    bind_recorders(0);
    int32_t par[9] = {bd, w, h, 3, chroma, BORDER, s->n, content, idx};
    put(nm("r%d_par", idx, 0), 'i', 1, 9, 0, par);
    put(nm("r%d_blocks", idx, 0), 'i', 2, (uint32_t)s->n, NBCOLS, rec);
    if (hbd) {
        put(nm("r%d_edges", idx, 0), 'H', 1, (uint32_t)n_edges, 0, edges), put(nm("r%d_prep", idx, 0), 'H', 1, (uint32_t)n_edges, 0, prep);
    } else {
        uint8_t *e8 = malloc(n_edges + 1), *p8 = malloc(n_edges + 1);
        for (int i = 0; i < n_edges; i++) e8[i] = (uint8_t)edges[i], p8[i] = (uint8_t)prep[i];
        put(nm("r%d_edges", idx, 0), 'B', 1, (uint32_t)n_edges, 0, e8), put(nm("r%d_prep", idx, 0), 'B', 1, (uint32_t)n_edges, 0, p8);
        free(e8), free(p8);
    }
    put(nm("r%d_sse", idx, 0), 'q', 2, (uint32_t)s->n, 4, sse);
    for (int p = 0; p < (chroma ? 3 : 1); p++) put(nm("r%d_pred%d", idx, p), hbd ? 'H' : 'B', 2, (uint32_t)(h >> (p > 0)), (uint32_t)(w >> (p > 0)), pb[p]);
    for (int p = 0; p < 3; p++) free(pb[p]);
    for (int r = 0; r < 3; r++) ref_free(&refs[r]);
    free(rec), free(edges), free(prep), free(sse), free(tb), free(src16), free(src8);
}

/* ---- the blend records ---- */
void svt_aom_blend_a64_mask_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, int, int, int, int);
void svt_aom_highbd_blend_a64_mask_8bit_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, int, int,
                                               int, int, int);
/* the one helper that source calls and the C-only library does not carry: a copy */
void svt_memcpy_intrin_sse(void *dst, void const *src, size_t size) { memcpy(dst, src, size); }
static int g_simd;

static int gen_blends(void) {
    static const int sizes[12][2] = {{1, 1}, {1, 128}, {128, 1}, {2, 64}, {64, 2}, {4, 4}, {8, 8}, {16, 32}, {32, 16}, {32, 32}, {128, 128}, {4, 16}};
    int k = 0;
    for (int hbd = 0; hbd < 2; hbd++)
        for (int sub = 0; sub < 4; sub++)
            for (int si = 0; si < 12; si++, k++) {
                const int      w = sizes[si][0], h = sizes[si][1], subw = sub & 1, subh = sub >> 1, mw = w << subw, mh = h << subh;
                const int      bd = !hbd ? 8 : (k & 1) ? 12 : 10, n = w * h, ext = k % 3 == 2;
                const uint64_t seed = 0x4949000000400000ull + 16 * (uint64_t)k;
                uint16_t      *a = malloc(2 * n), *b = malloc(2 * n), *o = malloc(2 * n), *o2 = malloc(2 * n);
                uint8_t       *a8 = malloc(n), *b8 = malloc(n), *o8 = malloc(n), *o28 = malloc(n), *m = malloc((size_t)mw * mh);
                for (int i = 0; i < n; i++) {
                    a[i] = (uint16_t)(ext ? (1 << bd) - 1 : draw(seed, i, 1u << bd)), b[i] = (uint16_t)(ext ? 0 : draw(seed + 1, i, 1u << bd));
                    a8[i] = (uint8_t)a[i], b8[i] = (uint8_t)b[i];
                }
                for (int i = 0; i < mw * mh; i++) m[i] = (uint8_t)(ext ? (((i % mw) ^ (i / mw)) & 2 ? 0 : 64) : draw(seed + 2, i, 65));
                if (hbd) svt_aom_highbd_blend_a64_mask_c((uint8_t *)o, w, (uint8_t *)a, w, (uint8_t *)b, w, m, mw, w, h, subw, subh, bd);
                else svt_aom_blend_a64_mask_c(o8, w, a8, w, b8, w, m, mw, w, h, subw, subh);
                if (g_simd) {
                    memset(o2, 0xA5, 2 * n), memset(o28, 0xA5, n);
                    if (hbd) svt_aom_highbd_blend_a64_mask_8bit_sse4_1((uint8_t *)o2, w, (uint8_t *)a, w, (uint8_t *)b, w, m, mw, w, h, subw, subh, bd);
                    else svt_aom_blend_a64_mask_sse4_1(o28, w, a8, w, b8, w, m, mw, w, h, subw, subh);
                    if (hbd ? memcmp(o, o2, 2 * n) : memcmp(o8, o28, n))
                        fprintf(stderr, "sse4_1 != c: blend record %d (hbd %d, %dx%d, sub %d %d)\n", k, hbd, w, h, subw, subh), exit(3);
                }
                const int32_t par[8] = {hbd, w, h, subw, subh, bd, k, ext};
                put(nm("b%d_par", k, 0), 'i', 1, 8, 0, par);
                put(nm("b%d_out", k, 0), hbd ? 'H' : 'B', 2, (uint32_t)h, (uint32_t)w, hbd ? (void *)o : (void *)o8);
                free(a), free(b), free(o), free(o2), free(a8), free(b8), free(o8), free(o28), free(m);
            }
    int32_t nn = k;
    put("nblend", 'i', 1, 1, 0, &nn);
    return k;
}

/* ---- the intra records: every kind x the ten sizes x both depths, through the tables' own (_c) functions ---- */
static int gen_intras(void) {
    int k = 0;
    for (int hbd = 0; hbd < 2; hbd++)
        for (int kind = 0; kind < 7; kind++)
            for (int si = 0; si < 10; si++, k++) {
                const int      w = g_psizes[si][0], h = g_psizes[si][1], bd = hbd ? 10 : 8, ext = k % 5 == 4;
                const uint64_t seed = 0x4949000000500000ull + 16 * (uint64_t)k;
                const TxSize   t = tx_of(w, h);
                uint16_t       above[48], left[48], o[32 * 32];
                uint8_t        above8[48], left8[48], o8[32 * 32];
                for (int i = 0; i < 48; i++) { /* the predictors read above[-1 .. w), left[-1 .. h) at most: the arrays start at [8] */
                    above[i] = (uint16_t)(ext ? (1 << bd) - 1 : draw(seed, i, 1u << bd)), left[i] = (uint16_t)(ext ? (1 << bd) - 1 : draw(seed + 1, i, 1u << bd));
                    above8[i] = (uint8_t)above[i], left8[i] = (uint8_t)left[i];
                }
                if (hbd) (kind < 4 ? g_dch[kind == 0 || kind == 2][kind == 0 || kind == 1][t] : g_ebh[kind == 4 ? V_PRED : kind == 5 ? H_PRED : SMOOTH_PRED][t])(o, w, above + 8, left + 8, bd);
                else (kind < 4 ? g_dc[kind == 0 || kind == 2][kind == 0 || kind == 1][t] : g_eb[kind == 4 ? V_PRED : kind == 5 ? H_PRED : SMOOTH_PRED][t])(o8, w, above8 + 8, left8 + 8);
                const int32_t par[6] = {hbd, w, h, kind, bd, k};
                put(nm("i%d_par", k, 0), 'i', 1, 6, 0, par);
                put(nm("i%d_out", k, 0), hbd ? 'H' : 'B', 2, (uint32_t)h, (uint32_t)w, hbd ? (void *)o : (void *)o8);
            }
    int32_t nn = k;
    put("nintra", 'i', 1, 1, 0, &nn);
    return k;
}

static void scene_tiling(Scene *s) {
    memset(s, 0, sizeof *s);
    s->w = 96, s->h = 64;
    for (int k = 0; k < 18; k++) add_cell(s, g_tiling[k][0], g_tiling[k][1], g_tiling[k][2], g_tiling[k][3]);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    g_simd = __builtin_cpu_supports("sse4.1") ? 1 : 0;
    static Scene s;
    if (!strcmp(argv[1], "--time")) {
        /* scripts/interintra_perf.py's lists through the reference's C on one core: the 96 x 64 tiling repeated over the
         * picture (one record per tile: the predictor of a tile does not depend on its place), small MVs, half wedge; the time
         * inside svt_aom_inter_prediction, summed over the blocks */
        static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
        for (int k = 0; k < 2; k++) {
            const int bd = shapes[k][0], tiles = (shapes[k][1] / 96) * (shapes[k][2] / 64);
            Rng       r = {0x4949000000600000ull + k};
            g_ms_pred = 0;
            for (int t = 0; t < tiles; t++) {
                scene_tiling(&s);
                draw_cells(&s, &r);
                for (int j = 0; j < s.n; j++) {
                    Cell *c = &s.c[j];
                    c->mv[0] = (int)rng_below(&r, 129) - 64, c->mv[1] = (int)rng_below(&r, 129) - 64, c->wedge = j & 1;
                    c->hang_x = c->hang_y = 0, c->up = c->y > 0, c->left = c->x > 0;
                }
                gen_record(0, &s, bd, 1, 0);
            }
            printf("{\"workload\": \"%dx%d %d-bit 4:2:0, %d inter-intra blocks (the 96x64 tiling x %d), half wedge\", "
                   "\"inter_prediction_interintra_c_ms\": %.2f, \"reps\": 1}\n",
                   shapes[k][1], shapes[k][2], bd, tiles * 18, tiles, g_ms_pred);
        }
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    int n = 0;
    /* {bd, chroma, content}: the tiling with drawn modes, wedges, MVs and availability */
    static const int recs[][3] = {{8, 1, 0},  {10, 1, 0}, {8, 0, 0},  {10, 0, 0}, {8, 1, 0},  {10, 1, 0}, {8, 1, 1},  {10, 1, 2},
                                  {8, 1, 3},  {10, 1, 3}, {8, 1, 0},  {10, 1, 0}, {8, 1, 2},  {10, 1, 1}, {8, 1, 0},  {10, 1, 0},
                                  {8, 1, 0},  {10, 1, 0}, {8, 0, 3},  {10, 1, 0}};
    for (unsigned k = 0; k < sizeof recs / sizeof recs[0]; k++) {
        Rng r = {0x4949000000080000ull + k};
        scene_tiling(&s);
        draw_cells(&s, &r);
        gen_record(n++, &s, recs[k][0], recs[k][1], recs[k][2]);
    }
    /* a 64 x 64 picture of four 32x32 blocks and one of sixty-four 8x8 blocks would add nothing the tiling lacks; one small
     * picture whose single block touches all four edges does: 32 x 32, both depths */
    for (int k = 0; k < 2; k++) {
        Rng r = {0x49490000000A0000ull + k};
        memset(&s, 0, sizeof s);
        s.w = s.h = 32;
        add_cell(&s, 0, 0, 32, 32);
        draw_cells(&s, &r);
        gen_record(n++, &s, k ? 10 : 8, 1, 0);
    }
    const int nb = gen_blends(), ni = gen_intras();
    int32_t   nn = n;
    put("nrec", 'i', 1, 1, 0, &nn);
    put("counts", 'i', 1, NCOUNT, 0, g_counts);
    golden_close(&g);
    int missing = 0;
    for (int k = 0; k < NCOUNT; k++)
        if (!g_counts[k]) fprintf(stderr, "count %d is zero\n", k), missing++;
    if (missing) return 3;
    fprintf(stderr, "%d picture records, %d blend records, %d intra records; %s\n", n, nb, ni,
            g_simd ? "every blend record equal through the _sse4_1 functions" : "no SSE4.1 on this host: the _c functions only");
    return 0;
}
