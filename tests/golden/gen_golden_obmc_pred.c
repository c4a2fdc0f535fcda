/*
 * gen_golden_obmc_pred.c — writes tests/golden/obmc_pred.bin: the reference's OBMC prediction, svt_aom_inter_prediction
 * with is_compound = 0 and motion_mode = OBMC_CAUSAL (EbEncInterPrediction.c:4070, :4507, av1_inter_prediction_obmc :3774),
 * on deterministic pictures with a mode-info grid (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C as build() leaves it under oracle/_ref/enc (libsvtenc.so, the whole encoder in its C-only
 * configuration).  Run from the repository root (REF = the reference checkout; the binary goes outside the repository):
 *
 *   S=$REF/Source; C=$S/Lib/Common; INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$S/Lib/Encoder/Codec \
 *     -I$S/Lib/Encoder/C_DEFAULT -I$S/Lib/Encoder/Globals -I$REF/third_party/fastfeat -I$REF -Ioracle/_ref/enc/gen"
 *   mkdir -p /tmp/obmc_simd
 *   gcc -O2 -msse4.1 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 -I$C/ASM_SSSE3 \
 *     -I$C/ASM_SSE4_1 -c $C/ASM_SSE4_1/EbBlend_a64_mask_sse4.c -o /tmp/obmc_simd/EbBlend_a64_mask_sse4.o
 *   gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_obmc_pred.c /tmp/obmc_simd/*.o \
 *     -o /tmp/gen_golden_obmc_pred -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *   /tmp/gen_golden_obmc_pred tests/golden/obmc_pred.bin
 *   /tmp/gen_golden_obmc_pred --time   # scripts/obmc_pred_perf.py's shapes through the reference's C, one core
 *
 * SIMD: where the CPU has SSE4.1, every blend record is made a second time through the reference's _sse4_1 function and must
 * be equal, or the generator stops.  Depth mismatch: every counted case is computed both ways (gen_record) and must differ.
 *
 * A record is a picture: a tiling of AV1 blocks ("cells"), each intra, single-reference or compound, with an MV, a
 * reference and a dual filter; the grid of ModeInfo pointers the reference walks is built from it.  Every cell that may be
 * OBMC_CAUSAL (single reference, at least 8x8) is predicted through svt_aom_inter_prediction into the record's predictor
 * picture.  The neighbour lists are NOT restated: while a block is predicted the four RTCD pointers of the OBMC blends
 * (svt_aom_blend_a64_{v,h}mask, svt_aom_highbd_blend_a64_{v,h}mask_16bit) are bound to recorders that note, for the luma
 * plane, where along the edge and how long each blend of the reference's own walk was, and call the _c function.  The
 * mode info of each span comes from the walk as well: before the prediction svt_aom_precompute_obmc_data runs on the block with
 * the two svt_av1_calc_target_weighted_pred_* RTCD pointers bound to recorders, which note the offset, the length and the
 * neighbour's MbModeInfo that the walk hands them; the two recordings must agree.  At 8 bits that call's wsrc / mask are kept for
 * the first block of every size over the file (r<i>_wmidx the blocks' indices, r<i>_wsrc<j> i32[h][w], r<i>_wmask<j> i16[h][w]; the
 * source luma is draw(0x4F42000000200000 + 256 * i, y * w + x, 256), 0 for content 1 and 3, 255 for content 2).  The file
 * regenerates byte-identically.
 *
 * Reference pictures are "drawn" as gen_golden_compound.c's (seed 0x4F42000000100000 + 256 * i + 4 * r + p), or constant /
 * alternating by `content`; tests/obmc_pred_cases.py rebuilds them.
 *
 * Records (golden_io format):
 *   nrec; r<i>_par i32[9] {bd, w, h, n_refs, chroma, border, n_blocks, content, i}; r<i>_blocks i[n_blocks][67]: {x, y, w, h,
 *   ref, filter_x, filter_y, mv_x, mv_y, n_above, n_left}, then nb[8] x {rel, size, ref, filter_x, filter_y, mv_x, mv_y} (above in
 *   nb[0 ..), left in nb[4 ..)); r<i>_pred<p> [h][w] the predictor planes (0 where no block writes; luma only when chroma is 0).
 *   content 0 drawn, 1 all zero, 2 all max, 3 reference r = max / zero checkerboard of phase r, 4 noise over the picture AND
 *   its border (sample (x, y), also outside the picture, is draw(seed + p, (y + 160) * 4096 + x + 2048, 1 << bd)): a strip that
 *   the clamp leaves wholly in the border still shows where it was read.
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
#include "EbModeDecisionProcess.h"
#include "EbReferenceObject.h"
#include "EbUtility.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "golden_io.h"

#define BORDER 80
#define PAD 160
#define MAXC 4096 /* cells of a scene: the 4K timing scene has 3795 */

enum { /* counts[] */
    C_SIZE8 = 0,           /* 17: size k predicted at 8 bits with chroma */
    C_SIZE10 = 17,         /* 17: at 10 bits (with or without chroma) */
    C_SIZE10C = 34,        /* 17: at 10 bits with chroma */
    C_SIZE_NOCHROMA = 51,  /* 17: without chroma */
    C_FX = 68, C_FY = 72,  /* 4 + 4: a span's filter kinds */
    C_NA = 76, C_NL = 81,  /* 5 + 5: n_above, n_left = 0 .. 4 */
    C_STOPPED = 86,        /* the walk stopped at the maximum with overlappable neighbours left */
    C_GAP = 87,            /* an intra neighbour left a gap */
    C_WIDER = 88,          /* a neighbour wider (taller) than the block that begins before it */
    C_PAIR4 = 89,          /* a pair of 4-wide (4-high) neighbours taken as one span */
    C_ROW0 = 90, C_COL0 = 91, C_RIGHT = 92, C_BOTTOM = 93,
    C_MISMATCH = 94,       /* 4: chroma of 32x8 above; of 8x8, 8x16, 8x32 left: the strip's clamp cuts on the far side where
                              the extent >> 1 clamp would cut earlier */
    C_TAP4 = 98,           /* 4: left luma of width 8; above luma of height 8; chroma of an 8-wide above span; of an 8-high
                              left span: non-zero phase, a kind with a 4-tap table */
    C_COMPOUND_NB = 102,   /* a compound neighbour */
    C_LO = 103, C_HI = 104, /* a blended block reaching 0 / the maximum */
    C_WS_ZERO = 105, C_WS_MAX = 106, C_WS_NEG = 107, /* a wsrc entry of 0, of 255 * 4096, below zero */
    NCOUNT = 108
};
static int32_t g_counts[NCOUNT];
static int     g_chroma; /* the record being made has chroma */
static int     g_wm_seen[17]; /* wsrc / mask are kept for the first 8-bit block of every size over the file */
static double  g_ms_pred, g_ms_pre; /* --time: inside svt_aom_inter_prediction / svt_aom_precompute_obmc_data */
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
static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}
static const int g_sizes[17][2] = {{8, 8},   {8, 16},  {16, 8},  {8, 32},  {32, 8},  {16, 16},  {16, 32},  {32, 16},  {16, 64},
                                   {64, 16}, {32, 32}, {32, 64}, {64, 32}, {64, 64}, {64, 128}, {128, 64}, {128, 128}};
static int size_index(int w, int h) {
    for (int k = 0; k < 17; k++)
        if (g_sizes[k][0] == w && g_sizes[k][1] == h) return k;
    return -1;
}

void svt_aom_asm_set_convolve_asm_table(void);
void svt_aom_asm_set_convolve_hbd_asm_table(void);

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

/* ---- the reference's structures ---- */
static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_ppcs;
static PictureControlSet       *g_pcs;
static Av1Common               *g_cm;
static EbPictureBufferDesc      g_enh;
static ModeDecisionContext     *g_md;
static EbObjectWrapper          g_wrap[3];
static EbReferenceObject        g_refobj[3];
static const MvReferenceFrame   g_frame_of[3] = {LAST_FRAME, LAST2_FRAME, BWDREF_FRAME}; /* (list, index) (0, 0), (0, 1), (1, 0) */

static void setup_reference(int w, int h) {
    if (!g_scs) {
        svt_aom_setup_common_rtcd_internal(0);
        svt_aom_setup_rtcd_internal(0);
        svt_aom_asm_set_convolve_asm_table();
        svt_aom_asm_set_convolve_hbd_asm_table();
        svt_aom_build_blk_geom(GEOM_7);
        g_scs = calloc(1, sizeof *g_scs), g_ppcs = calloc(1, sizeof *g_ppcs), g_pcs = calloc(1, sizeof *g_pcs);
        g_cm = calloc(1, sizeof *g_cm), g_md = calloc(1, sizeof *g_md);
        g_md->obmc_buff_0 = malloc(2 * MAX_MB_PLANE * MAX_SB_SQUARE), g_md->obmc_buff_1 = malloc(2 * MAX_MB_PLANE * MAX_SB_SQUARE);
        g_md->wsrc_buf = malloc(sizeof(int32_t) * MAX_SB_SQUARE), g_md->mask_buf = malloc(sizeof(int32_t) * MAX_SB_SQUARE);
        g_md->obmc_ctrls.max_blk_size_to_refine = 128, g_md->hbd_md = 0;
        g_pcs->ppcs = g_ppcs, g_pcs->scs = g_scs, g_ppcs->scs = g_scs, g_ppcs->is_not_scaled = 1;
        g_ppcs->av1_cm = g_cm, g_ppcs->enhanced_pic = &g_enh;
        g_scs->seq_header.sb_size = BLOCK_128X128;
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
    if (content == 4) return (int)draw(seed, (uint64_t)(y + PAD) * 4096 + (uint64_t)(x + 2048), maxv + 1);
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
                const uint16_t v = content == 4 ? (uint16_t)pic_value(bd, seed + p, pw, x, y, 4, ri)
                                                : r->p16[p][(clampi(y, 0, ph - 1) + pad) * st + clampi(x, 0, pw - 1) + pad];
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
    int x, y, w, h, kind /* 0 intra, 1 single, 2 compound */, ref, mv[2], fx, fy;
} Cell;
typedef struct Scene {
    int  w, h, n;
    Cell c[MAXC];
} Scene;
static BlockSize bsize_of(int w, int h) {
    for (int b = 0; b < BlockSizeS_ALL; b++)
        if (block_size_wide[b] == w && block_size_high[b] == h) return (BlockSize)b;
    fprintf(stderr, "no block size %dx%d\n", w, h), exit(3);
}
static uint32_t find_mds(int w, int h) {
    for (uint32_t k = 0; k < MAX_NUM_BLOCKS_ALLOC; k++) {
        const BlockGeom *g = get_blk_geom_mds(k);
        if (g->bwidth == w && g->bheight == h && g->has_uv) return k;
    }
    fprintf(stderr, "no block geometry of %dx%d\n", w, h), exit(3);
}
static void add_cell(Scene *s, int x, int y, int w, int h) {
    if (s->n >= MAXC) fprintf(stderr, "scene: too many cells\n"), exit(3);
    Cell *c = &s->c[s->n++];
    memset(c, 0, sizeof *c);
    c->x = x, c->y = y, c->w = w, c->h = h, c->kind = 1;
}
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
static void draw_cells(Scene *s, Rng *r, int intra_of, int comp_of) {
    for (int k = 0; k < s->n; k++) {
        Cell *c = &s->c[k];
        c->kind = (intra_of && rng_below(r, intra_of) == 0) ? 0 : (comp_of && rng_below(r, comp_of) == 0) ? 2 : 1;
        c->ref = (int)rng_below(r, 3), c->fx = (int)rng_below(r, 4), c->fy = (int)rng_below(r, 4);
        c->mv[0] = draw_mv(r, s->w), c->mv[1] = draw_mv(r, s->h);
    }
}
/* the 256 x 192 tiling of gen_golden_compound.c: all 17 sizes */
static const int g_tiling[][4] = {
    {0, 0, 128, 128},   {128, 0, 128, 64},  {128, 64, 64, 128}, {192, 64, 64, 64},  {192, 128, 64, 32},  {192, 160, 32, 32},
    {224, 160, 32, 16}, {224, 176, 16, 16}, {240, 176, 8, 16},  {248, 176, 8, 8},   {248, 184, 8, 8},    {0, 128, 32, 64},
    {32, 128, 64, 32},  {32, 160, 64, 16},  {32, 176, 32, 8},   {32, 184, 32, 8},   {64, 176, 16, 16},   {80, 176, 16, 8},
    {80, 184, 16, 8},   {96, 128, 16, 64},  {112, 128, 16, 32}, {112, 160, 8, 32},  {120, 160, 8, 32}};
static void scene_tiling(Scene *s, int mirror) {
    memset(s, 0, sizeof *s);
    s->w = 256, s->h = 192;
    for (unsigned k = 0; k < sizeof g_tiling / sizeof g_tiling[0]; k++) {
        const int *t = g_tiling[k];
        /* mirrored: the tiling turned by 180 degrees, so that the large blocks have the small ones above and left of them */
        if (mirror) add_cell(s, 256 - t[0] - t[2], 192 - t[1] - t[3], t[2], t[3]);
        else add_cell(s, t[0], t[1], t[2], t[3]);
    }
}
/* a probe: the block w x h at (L, T) under a band of aw x T cells and beside a band of L x lh cells (T or L 0: no band; the
 * corner cell, where both bands exist, is L x T; aw > w or lh > h: that band is one cell over the corner and the block) */
static void scene_probe(Scene *s, int w, int h, int T, int L, int aw, int lh) {
    memset(s, 0, sizeof *s);
    s->w = L + w, s->h = T + h;
    const int wide = T && aw > w, tall = L && !wide && lh > h; /* one band cell that takes the corner too and begins before the block */
    if (T && L && !wide && !tall) add_cell(s, 0, 0, L, T);
    if (wide) add_cell(s, 0, 0, L + w, T);
    else if (T)
        for (int x = L; x < s->w; x += aw) add_cell(s, x, 0, aw, T);
    if (tall) add_cell(s, 0, 0, L, T + h);
    else if (L)
        for (int y = T; y < s->h; y += lh) add_cell(s, 0, y, L, lh);
    add_cell(s, L, T, w, h);
}

/* ---- the recorders ---- */
static struct {
    uint8_t *base, *lo, *hi; /* the block's luma origin in the predictor, the luma buffer's extent */
    int      stride, shift, n[2], rel[2][8], size[2][8];
} g_rec;
static void note(int dir, const void *dst, int w, int h) {
    const uint8_t *d = dst;
    if (d < g_rec.lo || d >= g_rec.hi) return; /* a chroma plane */
    const long off = (long)(d - g_rec.base) >> g_rec.shift;
    const int  row = (int)(off / g_rec.stride), col = (int)(off % g_rec.stride), k = g_rec.n[dir]++;
    if (k >= 8 || (dir ? col : row)) fprintf(stderr, "recorder: unexpected blend\n"), exit(3);
    g_rec.rel[dir][k] = (dir ? row : col) / 4, g_rec.size[dir][k] = (dir ? h : w) / 4;
}
static void rec_v8(uint8_t *dst, uint32_t ds, const uint8_t *s0, uint32_t s0s, const uint8_t *s1, uint32_t s1s, const uint8_t *m, int w, int h) {
    note(0, dst, w, h), svt_aom_blend_a64_vmask_c(dst, ds, s0, s0s, s1, s1s, m, w, h);
}
static void rec_h8(uint8_t *dst, uint32_t ds, const uint8_t *s0, uint32_t s0s, const uint8_t *s1, uint32_t s1s, const uint8_t *m, int w, int h) {
    note(1, dst, w, h), svt_aom_blend_a64_hmask_c(dst, ds, s0, s0s, s1, s1s, m, w, h);
}
static void rec_v16(uint16_t *dst, uint32_t ds, const uint16_t *s0, uint32_t s0s, const uint16_t *s1, uint32_t s1s, const uint8_t *m, int w, int h, int bd) {
    note(0, dst, w, h), svt_aom_highbd_blend_a64_vmask_16bit_c(dst, ds, s0, s0s, s1, s1s, m, w, h, bd);
}
static void rec_h16(uint16_t *dst, uint32_t ds, const uint16_t *s0, uint32_t s0s, const uint16_t *s1, uint32_t s1s, const uint8_t *m, int w, int h, int bd) {
    note(1, dst, w, h), svt_aom_highbd_blend_a64_hmask_16bit_c(dst, ds, s0, s0s, s1, s1s, m, w, h, bd);
}

/* the walk of svt_aom_precompute_obmc_data: its two RTCD visitors note what the walk hands them (offset, length, the
 * neighbour's mode info) and call the _c function */
static struct {
    const ModeInfo *mis;
    int             n[2], rel[2][8], size[2][8], cell[2][8];
} g_walk;
static void walk_note(int dir, int rel, int size, const MbModeInfo *nb) {
    const int k = g_walk.n[dir]++;
    if (k >= 8) fprintf(stderr, "walk: too many neighbours\n"), exit(3);
    g_walk.rel[dir][k] = rel, g_walk.size[dir][k] = size, g_walk.cell[dir][k] = (int)((const ModeInfo *)nb - g_walk.mis);
}
static void walk_above(uint8_t is16bit, MacroBlockD *xd, int rel, uint8_t size, MbModeInfo *nb, void *fc, const int np) {
    walk_note(0, rel, size, nb), svt_av1_calc_target_weighted_pred_above_c(is16bit, xd, rel, size, nb, fc, np);
}
static void walk_left(uint8_t is16bit, MacroBlockD *xd, int rel, uint8_t size, MbModeInfo *nb, void *fc, const int np) {
    walk_note(1, rel, size, nb), svt_av1_calc_target_weighted_pred_left_c(is16bit, xd, rel, size, nb, fc, np);
}

/* ---- counters that need arithmetic ---- */
static int clamp_hi(int org, int extent, int spel_size, int dim, int ss) {
    return ((dim - extent - org) * 8) * (1 << (1 - ss)) + ((4 + spel_size) << 4) - 16;
}
static void count_span(const Scene *s, const Cell *b, int dir, int rel, int size, const Cell *nb) {
    const int side = dir ? b->w : b->h, org = dir ? b->x : b->y, dim = dir ? s->w : s->h;
    const int mv_across = nb->mv[dir ? 0 : 1], mv_along = nb->mv[dir ? 1 : 0], k_across = dir ? nb->fx : nb->fy, k_along = dir ? nb->fy : nb->fx;
    g_counts[C_FX + nb->fx]++, g_counts[C_FY + nb->fy]++;
    /* depth mismatch: chroma, side 8: extent min(side / 2, 32) = 4 luma = 2 chroma, predicted 4 */
    if (g_chroma && side == 8 && !(dir == 0 && (b->w == 8 || b->w == 16))) {
        const int q = (int16_t)mv_across, hi = clamp_hi(org, 4, 4, dim, 1), plain = clamp_hi(org, 4, 2, dim, 1);
        const int idx = dir == 0 ? 0 : b->h == 8 ? 1 : b->h == 16 ? 2 : 3;
        if (q > plain && hi != plain && (b->w == 32 || dir)) g_counts[C_MISMATCH + idx]++;
    }
    /* 4-tap strips with a phase at which the tables differ (not bilinear: it has no 4-tap table) */
    if (side == 8 && (mv_across & 7) && k_across != 3 && abs(mv_across) < 64) g_counts[C_TAP4 + (dir ? 0 : 1)]++;
    if (g_chroma && size == 2 && (mv_along & 15) && k_along != 3 && abs(mv_along) < 64 && !(dir == 0 && b->w * b->h <= 128)) g_counts[C_TAP4 + (dir ? 3 : 2)]++;
    g_counts[C_COMPOUND_NB] += nb->kind == 2;
    if (size * 4 == (dir ? b->h : b->w) && (dir ? nb->y < b->y : nb->x < b->x)) g_counts[C_WIDER]++;
    if ((dir ? nb->h : nb->w) == 4) g_counts[C_PAIR4]++;
}

/* one record: every OBMC-capable cell of the scene predicted */
static void gen_record(int idx, const Scene *s, int bd, int chroma, int content) {
    const int w = s->w, h = s->h, hbd = bd > 8, mi_cols = w / 4, mi_rows = h / 4;
    setup_reference(w, h);
    g_chroma = chroma;
    RefPic              refs[3];
    EbPictureBufferDesc rd[3], pd;
    for (int r = 0; r < 3; r++) {
        ref_alloc(&refs[r], bd, w, h, 0x4F42000000100000ull + 256 * (uint64_t)idx + 4 * r, content, r);
        ref_desc(&rd[r], &refs[r], bd, w, h);
        g_refobj[r].reference_picture = &rd[r];
    }
    /* the grid */
    ModeInfo  *mis = calloc(s->n, sizeof *mis);
    ModeInfo **grid = calloc((size_t)mi_cols * mi_rows, sizeof *grid);
    int       *cell_at = malloc(sizeof(int) * mi_cols * mi_rows);
    for (int i = 0; i < mi_cols * mi_rows; i++) cell_at[i] = -1;
    for (int k = 0; k < s->n; k++) {
        const Cell      *c = &s->c[k];
        BlockModeInfoEnc *m = &mis[k].mbmi.block_mi;
        m->bsize = bsize_of(c->w, c->h);
        m->ref_frame[0] = c->kind ? g_frame_of[c->ref] : INTRA_FRAME;
        m->ref_frame[1] = c->kind == 2 ? ALTREF_FRAME : (c->kind ? NONE_FRAME : NONE_FRAME);
        m->mv[0].as_mv.col = (int16_t)c->mv[0], m->mv[0].as_mv.row = (int16_t)c->mv[1];
        m->mv[1].as_mv.col = (int16_t)(c->mv[1] + 3), m->mv[1].as_mv.row = (int16_t)(c->mv[0] - 5); /* never read by OBMC */
        m->interp_filters = av1_make_interp_filters((InterpFilter)c->fy, (InterpFilter)c->fx);
        for (int y = c->y / 4; y < (c->y + c->h) / 4; y++)
            for (int x = c->x / 4; x < (c->x + c->w) / 4; x++) {
                if (cell_at[y * mi_cols + x] >= 0) fprintf(stderr, "scene %d: cells overlap\n", idx), exit(3);
                grid[y * mi_cols + x] = &mis[k], cell_at[y * mi_cols + x] = k;
            }
    }
    for (int i = 0; i < mi_cols * mi_rows; i++)
        if (cell_at[i] < 0) fprintf(stderr, "scene %d: a hole in the tiling\n", idx), exit(3);
    /* the predictor picture */
    uint8_t *pb[3];
    memset(&pd, 0, sizeof pd);
    for (int p = 0; p < 3; p++) pb[p] = calloc((size_t)(w >> (p > 0)) * (h >> (p > 0)), hbd ? 2 : 1);
    pd.buffer_y = pb[0], pd.buffer_cb = pb[1], pd.buffer_cr = pb[2];
    pd.stride_y = (uint16_t)w, pd.stride_cb = pd.stride_cr = (uint16_t)(w / 2), pd.width = (uint16_t)w, pd.height = (uint16_t)h;
    pd.bit_depth = bd > 8 ? EB_TEN_BIT : EB_EIGHT_BIT;
    svt_av1_calc_target_weighted_pred_above = walk_above, svt_av1_calc_target_weighted_pred_left = walk_left;
    /* the source picture of the weighted source: 8-bit luma, drawn (content 0, 4), zero (1, 3) or 255 (2) */
    uint8_t *srcp = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++)
        srcp[i] = (uint8_t)(content == 2 ? 255 : (content == 1 || content == 3) ? 0 : draw(0x4F42000000200000ull + 256 * (uint64_t)idx, i, 256));
    g_enh.buffer_y = srcp, g_enh.stride_y = (uint16_t)w, g_enh.org_x = g_enh.org_y = 0;
    int n_wm = 0;
    int32_t wm_idx[17];
    svt_aom_blend_a64_vmask = rec_v8, svt_aom_blend_a64_hmask = rec_h8;
    svt_aom_highbd_blend_a64_vmask_16bit = rec_v16, svt_aom_highbd_blend_a64_hmask_16bit = rec_h16;

    int32_t *rec = calloc((size_t)s->n * 67, sizeof(int32_t));
    int      nb_out = 0;
    for (int k = 0; k < s->n; k++) {
        const Cell *c = &s->c[k];
        if (c->kind != 1 || c->w < 8 || c->h < 8) continue;
        BlkStruct   blk;
        MacroBlockD xd;
        MvUnit      mvu;
        memset(&blk, 0, sizeof blk), memset(&xd, 0, sizeof xd), memset(&mvu, 0, sizeof mvu);
        blk.av1xd = &xd, blk.mds_idx = (uint16_t)find_mds(c->w, c->h);
        xd.mb_to_top_edge = -(c->y * 8), xd.mb_to_bottom_edge = (h - c->h - c->y) * 8;
        xd.mb_to_left_edge = -(c->x * 8), xd.mb_to_right_edge = (w - c->w - c->x) * 8;
        xd.n4_w = (uint8_t)(c->w / 4), xd.n4_h = (uint8_t)(c->h / 4), xd.n8_w = (uint8_t)(c->w / 8), xd.n8_h = (uint8_t)(c->h / 8);
        xd.mi_stride = mi_cols, xd.mi = grid + (c->y / 4) * mi_cols + c->x / 4;
        xd.up_available = c->y > 0, xd.left_available = c->x > 0;
        xd.mi_row = c->y / 4, xd.mi_col = c->x / 4;
        mvu.pred_direction = UNI_PRED_LIST_0;
        mvu.mv[REF_LIST_0].x = (int16_t)c->mv[0], mvu.mv[REF_LIST_0].y = (int16_t)c->mv[1];
        /* svt_aom_precompute_obmc_data: the walk's record, and at 8 bits wsrc / mask (at 10 bits the 8-bit path runs over the
         * references' upper 8 bits: only its walk is kept) */
        memset(&g_walk, 0, sizeof g_walk);
        g_walk.mis = mis;
        g_md->blk_geom = get_blk_geom_mds(blk.mds_idx), g_md->blk_ptr = &blk, g_md->blk_org_x = (uint16_t)c->x, g_md->blk_org_y = (uint16_t)c->y;
        double t0 = now_ms();
        svt_aom_precompute_obmc_data(g_pcs, g_md);
        g_ms_pre += now_ms() - t0;
        const int si_w = size_index(c->w, c->h);
        if (!hbd && si_w >= 0 && !g_wm_seen[si_w]++) {
            int16_t *m16 = malloc(sizeof(int16_t) * c->w * c->h);
            for (int i = 0; i < c->w * c->h; i++) {
                m16[i] = (int16_t)g_md->mask_buf[i];
                g_counts[C_WS_ZERO] += g_md->wsrc_buf[i] == 0, g_counts[C_WS_MAX] += g_md->wsrc_buf[i] == 255 * 4096, g_counts[C_WS_NEG] += g_md->wsrc_buf[i] < 0;
            }
            put(nm("r%d_wsrc%d", idx, n_wm), 'i', 2, (uint32_t)c->h, (uint32_t)c->w, g_md->wsrc_buf);
            put(nm("r%d_wmask%d", idx, n_wm), 'h', 2, (uint32_t)c->h, (uint32_t)c->w, m16);
            wm_idx[n_wm++] = nb_out;
            free(m16);
        }
        memset(&g_rec, 0, sizeof g_rec);
        g_rec.shift = hbd, g_rec.stride = w, g_rec.lo = pb[0], g_rec.hi = pb[0] + ((size_t)w * h << hbd);
        g_rec.base = pb[0] + (((size_t)c->y * w + c->x) << hbd);
        MvReferenceFrame rf[2] = {g_frame_of[c->ref], NONE_FRAME};
#define PREDICT()                                                                                                                 \
    svt_aom_inter_prediction(g_scs, g_pcs, av1_make_interp_filters((InterpFilter)c->fy, (InterpFilter)c->fx), &blk,              \
                             (uint8_t)av1_ref_frame_type(rf), &mvu, 0, OBMC_CAUSAL, 0, NULL, 1, NULL, NULL, NULL, NULL, 0, 0, 0, 0, \
                             (uint16_t)c->x, (uint16_t)c->y, (uint8_t)c->w, (uint8_t)c->h, &rd[c->ref], NULL, &pd, (uint16_t)c->x, \
                             (uint16_t)c->y, chroma ? PICTURE_BUFFER_DESC_FULL_MASK : PICTURE_BUFFER_DESC_LUMA_MASK, (uint8_t)bd, hbd)
        t0 = now_ms();
        PREDICT();
        g_ms_pred += now_ms() - t0;
        int mismatch_before = 0, mismatch_was[4];
        for (int q = 0; q < 4; q++) mismatch_was[q] = g_counts[C_MISMATCH + q], mismatch_before += mismatch_was[q];
        int32_t *o = rec + 67 * nb_out++;
        const int32_t head[11] = {c->x, c->y, c->w, c->h, c->ref, c->fx, c->fy, c->mv[0], c->mv[1], g_rec.n[0], g_rec.n[1]};
        memcpy(o, head, sizeof head);
        const int si = size_index(c->w, c->h);
        if (si < 0 || g_rec.n[0] > 4 || g_rec.n[1] > 4) fprintf(stderr, "record %d: block %d\n", idx, k), exit(3);
        g_counts[(hbd ? C_SIZE10 : C_SIZE8) + si] += hbd || chroma, g_counts[C_SIZE10C + si] += hbd && chroma;
        g_counts[C_SIZE_NOCHROMA + si] += !chroma;
        g_counts[C_NA + g_rec.n[0]]++, g_counts[C_NL + g_rec.n[1]]++;
        g_counts[C_ROW0] += c->y == 0, g_counts[C_COL0] += c->x == 0, g_counts[C_RIGHT] += c->x + c->w == w, g_counts[C_BOTTOM] += c->y + c->h == h;
        for (int dir = 0; dir < 2; dir++) {
            int covered = 0, inter = 0; /* 4-sample units of the edge under a span / under an inter neighbour */
            for (int j = 0; j < g_rec.n[dir]; j++) {
                const int rel = g_rec.rel[dir][j], size = g_rec.size[dir][j], ci = g_walk.cell[dir][j];
                if (g_walk.n[dir] != g_rec.n[dir] || g_walk.rel[dir][j] != rel || g_walk.size[dir][j] != size || ci < 0 || ci >= s->n)
                    fprintf(stderr, "record %d: the precompute walk and the prediction's blends disagree\n", idx), exit(3);
                const Cell   *n = &s->c[ci];
                const int32_t v[7] = {rel, size, n->ref, n->fx, n->fy, n->mv[0], n->mv[1]};
                if (n->kind == 0) fprintf(stderr, "record %d: an intra cell under a span\n", idx), exit(3);
                memcpy(o + 11 + 7 * (4 * dir + j), v, sizeof v);
                count_span(s, c, dir, rel, size, n);
                covered += size;
            }
            if (dir ? c->x > 0 : c->y > 0)
                for (int u = 0; u < (dir ? c->h : c->w) / 4; u++) {
                    const int ci = dir ? cell_at[(c->y / 4 + u) * mi_cols + c->x / 4 - 1] : cell_at[(c->y / 4 - 1) * mi_cols + c->x / 4 + u];
                    inter += s->c[ci].kind != 0;
                    g_counts[C_GAP] += s->c[ci].kind == 0 && u > 0 && g_rec.n[dir];
                }
            g_counts[C_STOPPED] += g_rec.n[dir] == 4 && inter > covered + 1;
        }
        /* A depth-mismatch case was counted: compute both.  The block again with the across component of its neighbours' MVs
         * cut to the bound that the extent >> 1 clamp would use (the reference's own, wider clamp then leaves it alone, so the
         * chroma strip is read where that clamp would read it); the case counts only if the block's chroma comes out different
         * (the generator stops at the end unless each of the four cases counted).  Then the record's own samples are put back. */
        int mismatch_after = 0;
        for (int q = 0; q < 4; q++) mismatch_after += g_counts[C_MISMATCH + q];
        if (mismatch_after > mismatch_before) {
            uint8_t *keep[3];
            int16_t  old[2][8];
            for (int p = 0; p < 3; p++) {
                const size_t bytes = (size_t)(w >> (p > 0)) * (h >> (p > 0)) << hbd;
                keep[p] = malloc(bytes), memcpy(keep[p], pb[p], bytes);
            }
            for (int dir = 0; dir < 2; dir++)
                for (int j = 0; j < g_walk.n[dir]; j++) {
                    MV       *mv = &mis[g_walk.cell[dir][j]].mbmi.block_mi.mv[0].as_mv;
                    int16_t  *comp = dir ? &mv->col : &mv->row;
                    const int plain = clamp_hi(dir ? c->x : c->y, 4, 2, dir ? w : h, 1);
                    old[dir][j] = *comp;
                    if ((dir ? c->w : c->h) == 8 && *comp > plain) *comp = (int16_t)plain;
                }
            memset(g_rec.n, 0, sizeof g_rec.n);
            PREDICT();
            int differs = 0;
            for (int p = 1; p < 3; p++)
                for (int y = c->y / 2; y < (c->y + c->h) / 2; y++)
                    differs |= memcmp(pb[p] + (((size_t)y * (w / 2) + c->x / 2) << hbd), keep[p] + (((size_t)y * (w / 2) + c->x / 2) << hbd),
                                      (size_t)(c->w / 2) << hbd) != 0;
            if (!differs) /* e.g. a strip wholly inside a replicated border: not a case, so not counted */
                for (int q = 0; q < 4; q++) g_counts[C_MISMATCH + q] = mismatch_was[q];
            for (int dir = 0; dir < 2; dir++)
                for (int j = 0; j < g_walk.n[dir]; j++) {
                    MV *mv = &mis[g_walk.cell[dir][j]].mbmi.block_mi.mv[0].as_mv;
                    *(dir ? &mv->col : &mv->row) = old[dir][j];
                }
            for (int p = 0; p < 3; p++) memcpy(pb[p], keep[p], (size_t)(w >> (p > 0)) * (h >> (p > 0)) << hbd), free(keep[p]);
        }
#undef PREDICT
        /* the clip ends of a blended block */
        if (o[9] + o[10]) {
            int lo = 65535, hi = 0;
            for (int y = c->y; y < c->y + c->h; y++)
                for (int x = c->x; x < c->x + c->w; x++) {
                    const int v = hbd ? ((uint16_t *)pb[0])[y * w + x] : pb[0][y * w + x];
                    lo = v < lo ? v : lo, hi = v > hi ? v : hi;
                }
            g_counts[C_LO] += lo == 0, g_counts[C_HI] += hi == (1 << bd) - 1;
        }
    }
    int32_t par[9] = {bd, w, h, 3, chroma, BORDER, nb_out, content, idx};
    put(nm("r%d_par", idx, 0), 'i', 1, 9, 0, par);
    put(nm("r%d_blocks", idx, 0), 'i', 2, (uint32_t)nb_out, 67, rec);
    put(nm("r%d_wmidx", idx, 0), 'i', 1, (uint32_t)n_wm, 0, wm_idx);
    free(srcp);
    for (int p = 0; p < (chroma ? 3 : 1); p++) put(nm("r%d_pred%d", idx, p), hbd ? 'H' : 'B', 2, (uint32_t)(h >> (p > 0)), (uint32_t)(w >> (p > 0)), pb[p]);
    for (int p = 0; p < 3; p++) free(pb[p]);
    for (int r = 0; r < 3; r++) ref_free(&refs[r]);
    free(rec), free(mis), free(grid), free(cell_at);
}

/* ---- the six blend functions: m<k>_par i32[6] {function, w, h, bd, k, 0}, m<k>_out [h][w].  function 0 vmask, 1 hmask (8
 * bits), 2 / 3 the _16bit forms, 4 / 5 the _8bit forms (16-bit samples behind a plain uint8_t * cast, as this encoder's C reads them; bd 10 for k even, 12 for k odd).  src0 is draw(seed, i, 1 << bd),
 * src1 draw(seed + 1, ...), the mask draw(seed + 2, i, 65), seed = 0x4F42000000300000 + 16 * k; every third record has the
 * extremes instead: src0 all max, src1 all zero, the mask 64, 0, 64, ... ---- */
/* the reference's SSE4.1 forms, compiled stand-alone from its tree (the build lines above) */
void svt_aom_blend_a64_vmask_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, int, int);
void svt_aom_blend_a64_hmask_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, int, int);
void svt_aom_highbd_blend_a64_vmask_16bit_sse4_1(uint16_t *, uint32_t, const uint16_t *, uint32_t, const uint16_t *, uint32_t, const uint8_t *, int, int, int);
void svt_aom_highbd_blend_a64_hmask_16bit_sse4_1(uint16_t *, uint32_t, const uint16_t *, uint32_t, const uint16_t *, uint32_t, const uint8_t *, int, int, int);
void svt_aom_highbd_blend_a64_vmask_8bit_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, int, int, int);
void svt_aom_highbd_blend_a64_hmask_8bit_sse4_1(uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, uint32_t, const uint8_t *, int, int, int);
/* the one helper that source calls and the C-only library does not carry: a copy */
void svt_memcpy_intrin_sse(void *dst, void const *src, size_t size) { memcpy(dst, src, size); }
static int g_simd; /* the CPU has SSE4.1: every blend record is made a second time through the _sse4_1 function */

static void gen_blends(void) {
    static const int sizes[10][2] = {{1, 1}, {1, 128}, {128, 1}, {2, 128}, {128, 2}, {8, 8}, {32, 4}, {4, 32}, {64, 16}, {16, 64}};
    int k = 0;
    for (int f = 0; f < 6; f++)
        for (int si = 0; si < 10; si++, k++) {
            const int      w = sizes[si][0], h = sizes[si][1], bd = f < 2 ? 8 : (k & 1) ? 12 : 10, n = w * h, ext = k % 3 == 2;
            const uint64_t seed = 0x4F42000000300000ull + 16 * (uint64_t)k;
            uint16_t      *a = malloc(2 * n), *b = malloc(2 * n), *o = malloc(2 * n);
            uint8_t       *a8 = malloc(n), *b8 = malloc(n), *o8 = malloc(n), m[128];
            for (int i = 0; i < n; i++) {
                a[i] = (uint16_t)(ext ? (1 << bd) - 1 : draw(seed, i, 1u << bd)), b[i] = (uint16_t)(ext ? 0 : draw(seed + 1, i, 1u << bd));
                a8[i] = (uint8_t)a[i], b8[i] = (uint8_t)b[i];
            }
            for (int i = 0; i < 128; i++) m[i] = (uint8_t)(ext ? ((i & 1) ? 0 : 64) : draw(seed + 2, i, 65));
            switch (f) {
            case 0: svt_aom_blend_a64_vmask_c(o8, w, a8, w, b8, w, m, w, h); break;
            case 1: svt_aom_blend_a64_hmask_c(o8, w, a8, w, b8, w, m, w, h); break;
            case 2: svt_aom_highbd_blend_a64_vmask_16bit_c(o, w, a, w, b, w, m, w, h, bd); break;
            case 3: svt_aom_highbd_blend_a64_hmask_16bit_c(o, w, a, w, b, w, m, w, h, bd); break;
            case 4: svt_aom_highbd_blend_a64_vmask_8bit_c((uint8_t *)o, w, (uint8_t *)a, w, (uint8_t *)b, w, m, w, h, bd); break;
            default: svt_aom_highbd_blend_a64_hmask_8bit_c((uint8_t *)o, w, (uint8_t *)a, w, (uint8_t *)b, w, m, w, h, bd); break;
            }
            if (g_simd) {
                uint16_t *o2 = malloc(2 * n);
                uint8_t  *o28 = malloc(n);
                memset(o2, 0xA5, 2 * n), memset(o28, 0xA5, n);
                switch (f) {
                case 0: svt_aom_blend_a64_vmask_sse4_1(o28, w, a8, w, b8, w, m, w, h); break;
                case 1: svt_aom_blend_a64_hmask_sse4_1(o28, w, a8, w, b8, w, m, w, h); break;
                case 2: svt_aom_highbd_blend_a64_vmask_16bit_sse4_1(o2, w, a, w, b, w, m, w, h, bd); break;
                case 3: svt_aom_highbd_blend_a64_hmask_16bit_sse4_1(o2, w, a, w, b, w, m, w, h, bd); break;
                case 4: svt_aom_highbd_blend_a64_vmask_8bit_sse4_1((uint8_t *)o2, w, (uint8_t *)a, w, (uint8_t *)b, w, m, w, h, bd); break;
                default: svt_aom_highbd_blend_a64_hmask_8bit_sse4_1((uint8_t *)o2, w, (uint8_t *)a, w, (uint8_t *)b, w, m, w, h, bd); break;
                }
                if (f < 2 ? memcmp(o8, o28, n) : memcmp(o, o2, 2 * n))
                    fprintf(stderr, "sse4_1 != c: blend record %d (function %d, %dx%d)\n", k, f, w, h), exit(3);
                free(o2), free(o28);
            }
            const int32_t par[6] = {f, w, h, bd, k, ext};
            put(nm("m%d_par", k, 0), 'i', 1, 6, 0, par);
            put(nm("m%d_out", k, 0), f < 2 ? 'B' : 'H', 2, (uint32_t)h, (uint32_t)w, f < 2 ? (void *)o8 : (void *)o);
            free(a), free(b), free(o), free(a8), free(b8), free(o8);
        }
    int32_t nn = k;
    put("nblend", 'i', 1, 1, 0, &nn);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    g_simd = __builtin_cpu_supports("sse4.1") ? 1 : 0;
    static Scene s;
    if (!strcmp(argv[1], "--time")) {
        /* scripts/obmc_pred_perf.py's workloads through the reference's C on one core: the tiling repeated over the picture,
         * every cell single-reference with small MVs; the time inside the two reference entries, summed over the blocks */
        static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
        for (int k = 0; k < 2; k++) {
            const int bd = shapes[k][0], w = shapes[k][1] / 256 * 256, h = shapes[k][2] / 192 * 192;
            Rng       r = {0x4F42000000400000ull + k};
            memset(&s, 0, sizeof s);
            s.w = w, s.h = h;
            for (int ty = 0; ty < h / 192; ty++)
                for (int tx = 0; tx < w / 256; tx++)
                    for (unsigned j = 0; j < sizeof g_tiling / sizeof g_tiling[0]; j++)
                        add_cell(&s, g_tiling[j][0] + 256 * tx, g_tiling[j][1] + 192 * ty, g_tiling[j][2], g_tiling[j][3]);
            draw_cells(&s, &r, 0, 0);
            for (int j = 0; j < s.n; j++) s.c[j].mv[0] = (int)rng_below(&r, 129) - 64, s.c[j].mv[1] = (int)rng_below(&r, 129) - 64;
            g_ms_pred = g_ms_pre = 0;
            gen_record(0, &s, bd, 1, 0);
            printf("{\"workload\": \"%dx%d %d-bit 4:2:0, %d OBMC_CAUSAL blocks over %dx%d, every block with the neighbours its grid gives\", "
                   "\"inter_prediction_obmc_c_ms\": %.2f, \"precompute_obmc_data_c_ms\": %.2f, \"reps\": 1}\n",
                   shapes[k][1], shapes[k][2], bd, s.n, w, h, g_ms_pred, g_ms_pre);
        }
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    int   n = 0;
    /* the batch records: the 256 x 192 tiling and its mirror image, some cells intra, some compound */
    for (int i = 0; i < 2; i++) {
        Rng r = {0x4F42000000080000ull + i};
        scene_tiling(&s, i);
        draw_cells(&s, &r, 7, 6);
        int seen[17] = {0}; /* the first cell of every size stays single-reference: the record holds all 17 */
        for (int j = 0; j < s.n; j++)
            if (!seen[size_index(s.c[j].w, s.c[j].h)]++) s.c[j].kind = 1;
        gen_record(n++, &s, 8, !i, 0); /* the second without chroma */
    }
    /* probes: {w, h, T, L, aw, lh, bd, chroma, content, intra_of}: one block under and beside bands of small cells */
    static const int probes[][10] = {
        {8, 8, 8, 8, 8, 8, 10, 1, 0, 0},     {8, 8, 8, 8, 4, 4, 8, 1, 0, 0},      {8, 16, 8, 8, 8, 8, 10, 1, 0, 0},   {16, 8, 8, 8, 4, 8, 10, 1, 0, 0},
        {8, 32, 16, 8, 8, 8, 10, 1, 0, 0},   {32, 8, 8, 16, 8, 8, 10, 1, 0, 0},   {32, 8, 8, 16, 8, 4, 8, 1, 0, 0},   {16, 16, 8, 8, 8, 4, 10, 1, 0, 0},
        {16, 32, 8, 16, 8, 8, 10, 1, 0, 3},  {32, 16, 16, 8, 8, 8, 10, 1, 0, 3},  {16, 64, 16, 16, 16, 8, 10, 1, 0, 4}, {64, 16, 8, 16, 8, 8, 10, 1, 0, 0},
        {32, 32, 8, 8, 8, 8, 10, 1, 0, 4},   {32, 64, 8, 8, 8, 8, 10, 1, 0, 5},   {64, 32, 8, 8, 8, 8, 10, 1, 0, 5},  {64, 64, 8, 8, 8, 8, 10, 1, 0, 6},
        {64, 16, 8, 0, 8, 8, 8, 1, 0, 0},    {16, 64, 0, 8, 8, 8, 8, 0, 0, 0},    {16, 16, 16, 16, 32, 16, 8, 1, 0, 0}, {16, 16, 16, 16, 16, 32, 10, 1, 0, 0}, {8, 8, 8, 8, 8, 8, 8, 1, 1, 0},
        {16, 16, 8, 8, 8, 8, 10, 1, 2, 0},   {16, 16, 8, 8, 8, 8, 8, 1, 3, 0},    {32, 32, 8, 8, 16, 16, 10, 1, 3, 0}};
    for (unsigned k = 0; k < sizeof probes / sizeof probes[0]; k++) {
        const int *p = probes[k];
        Rng        r = {0x4F42000000090000ull + k};
        scene_probe(&s, p[0], p[1], p[2], p[3], p[4], p[5]);
        draw_cells(&s, &r, p[9], 5);
        s.c[s.n - 1].kind = 1; /* the block itself is single-reference */
        gen_record(n++, &s, p[6], p[7], p[8]);
    }
    /* the blocks with a side of 8, at both depths, over noise that goes on into the border: variant 0 small MVs of odd
     * eighths (the 4-tap strips), variant 1 MVs that the strip's clamp cuts on the far side (the depth-mismatch chroma) */
    static const int eight[4][2] = {{8, 8}, {8, 16}, {8, 32}, {32, 8}};
    for (int k = 0; k < 16; k++) {
        Rng r = {0x4F420000000B0000ull + k};
        scene_probe(&s, eight[k & 3][0], eight[k & 3][1], 8, 8, 8, 8);
        draw_cells(&s, &r, 0, 0);
        for (int j = 0; j < s.n - 1; j++) {
            Cell *c = &s.c[j];
            c->fx = (j + k) % 3, c->fy = (j + k + 1) % 3;
            c->mv[0] = (k & 8) ? 8 * (s.w + 60) + 3 : 2 * (int)rng_below(&r, 7) + 1 + ((j & 1) ? 16 : -16);
            c->mv[1] = (k & 8) ? 8 * (s.h + 60) + 5 : 2 * (int)rng_below(&r, 7) + 1 + ((j & 1) ? -8 : 8);
        }
        gen_record(n++, &s, (k & 4) ? 10 : 8, 1, 4);
    }
    {
        static const int big[4][4] = {{0, 0, 128, 128}, {128, 0, 64, 128}, {0, 128, 128, 64}, {128, 128, 64, 64}};
        Rng r = {0x4F420000000C0000ull};
        memset(&s, 0, sizeof s);
        s.w = 192, s.h = 192;
        for (int k = 0; k < 4; k++) add_cell(&s, big[k][0], big[k][1], big[k][2], big[k][3]);
        draw_cells(&s, &r, 0, 0);
        gen_record(n++, &s, 10, 1, 0);
    }
    gen_blends();
    int32_t nn = n;
    put("nrec", 'i', 1, 1, 0, &nn);
    put("counts", 'i', 1, NCOUNT, 0, g_counts);
    golden_close(&g);
    int missing = 0;
    for (int k = 0; k < NCOUNT; k++)
        if (!g_counts[k]) fprintf(stderr, "count %d is zero\n", k), missing++;
    if (missing) return 3;
    fprintf(stderr, "%d picture records, 60 blend records; %s\n", n,
            g_simd ? "every blend record equal through the _sse4_1 functions" : "no SSE4.1 on this host: the _c functions only");
    return 0;
}
