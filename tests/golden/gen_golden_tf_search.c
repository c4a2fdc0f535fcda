/*
 * gen_golden_tf_search.c — writes tests/golden/tf_search.bin: the sub-pel motion search of the reference's temporal filter
 * (the `frame_index != index_center` section of produce_temporally_filtered_pic, EbTemporalFiltering.c:3087-3261: the four
 * tf_*_sub_pel_search walks, the 64-vs-32 test, the pred_error_32x32_th bypass, derive_tf_32x32_block_split_flag) on
 * deterministic inputs, and three chains search -> tf_*_inter_prediction -> convert_64x64_info_to_32x32_info -> filter (test
 * infrastructure; never shipped, not built by build()).
 *
 * Built and run as gen_golden_interp.c is (its header holds the recipe: the same include paths, the same AVX2 / SSSE3
 * convolve objects, oracle/_ref/enc/libsvtenc.so), with this file's name and tests/golden/tf_search.bin.
 * EbTemporalFiltering.c is included below, not linked: the functions called are static there.  The variance functions
 * are reached through svt_aom_mefn_ptr, whose vf / vf_hbd_10 entries of the eight block sizes the search uses are wrapped
 * to log every value: the generator replays each walk from the log (positions in the reference's order under its skip
 * rules), counts what happened, and stops if the replay does not consume the log exactly or does not end on the
 * reference's MV and error.
 *
 * SIMD: where the CPU has AVX2 every record is made a second time with the eight convolve RTCD pointers on the _avx2
 * functions and the vf / vf_hbd_10 entries on the functions the reference's RTCD picks with AVX2 (_avx2; _sse2 for the
 * 8-bit 8x8 and 8x4, which have no _avx2 form; the highbd 8x4 has the C form only), and must be equal, or the generator
 * stops.  Beside gen_golden_interp.c's objects the recipe compiles Lib/Encoder/ASM_AVX2/variance_avx2.c,
 * ASM_AVX2/highbd_variance_avx2.c and ASM_SSE2/variance_sse2.c the same way.
 *
 *   gen_golden_tf_search --time    scripts/tf_search_perf.py's shapes (1920x1080 8-bit, 3840x2160 10-bit, 6 references,
 *   region-wise whole-sample motion and noise, its own draw) through the reference's searches and partition decisions
 *   alone (no inter prediction), C and SIMD, on one core.
 *
 * Inputs (tests/tf_search_cases.py rebuilds them; draw(seed, i, mod) = SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) %
 * mod): pictures of 136x72, 64-aligned area 192x128, 2 references with 80 samples around them (luma; chroma halved).
 *   H, a texture on a half-sample grid of 736 x 608: H(u, v) = clamp((u + v) * sc / 8 + draw(S, (v >> 3) * 92 + (u >> 3),
 *     128 * sc) + draw(S + 1, v * 736 + u, 16 * sc)), sc = 1 << (bd - 8), S = 0x5453000000000000 + 16 * (bd > 8).
 *   centre luma (x, y) over the aligned area = H(2 * (x + 80) + 16, 2 * (y + 80) + 16).
 *   reference r luma (x, y), x in [-80, 216), y in [-80, 152): cell = ((y + 80) / 24) * 13 + (x + 80) / 24; per (r, cell)
 *     dx = draw(S + 2 + r, 4 * cell, 13) - 6, dy = draw(.., 4 * cell + 1, 13) - 6 (half samples), amp = {0, 2, 8, 24}[draw(..,
 *     4 * cell + 2, 4)] * sc; the value H(u + dx, v + dy) + (amp ? draw(S + 4 + r, (y + 80) * 296 + x + 80, 2 * amp + 1) - amp
 *     : 0), clamped.  Cell (3, 3) (x, y in [-8, 16)) is an exact copy moved by (1, 1): dx = 2, dy = 2, amp = 0.  Cells from 5
 *     of rows from 5 (x and y from 40) move together with little noise, dx = 2, dy = 0, amp = 2 * sc: whole 64x64
 *     blocks that match well.  Samples with x in [40, 88), y in [-32, 40) are flat: the value 100 * sc, and dx = dy = 0 for
 *     the full-pel draw.
 *   chroma (chains only): plane p of the centre draw(S + 8 + p, y * 96 + x, 64 * sc) + (2 * x + y) * sc / 4 over 96 x 64; of
 *     reference r draw(S + 10 + 2 * r + p, (y + 40) * 148 + x + 40, 64 * sc) + (2 * x + y + 160) * sc / 4 over [-40, 108) x
 *     [-40, 76), clamped.
 *   8-bit planes of a 10-bit picture (use_8bit_subpel): sample >> 2.
 *   full-pel MVs: written to the file (f<d>_*), drawn near -floor(d / 2) of the cell under the block's centre (the content of
 *     the reference at x + d / 2 is the centre's at x), one component in sixteen far outside the picture; the
 *     64x64 and 32x32 blocks of the lower block row and the 16x16 / 8x8 blocks inside cell (3, 3) start exactly.
 *
 * Records (golden_io format):
 *   nset i32[1]; per bit depth d in {8, 10}: f<d>_mv64 h[2][6][2], _mv32 h[..][4][2], _mv16 h[..][16][2], _mv8 h[..][64][2]
 *   (x, y), nested raster indices.
 *   s<k>_par i32[12]  {bd, half, quarter, eighth, use_2tap, sub_sampling_shift, enable_8x8_pred, subpel_early_exit_th,
 *             n_refs, border, set, 0}; s<k>_th32 Q[1] pred_error_32x32_th; s<k>_force64 B[2][6]
 *   s<k>_use64 B[2][6], _mv64 h[..][2], _split32 B[..][4], _split16 B[..][16], _mv32 h[..][4][2], _mv16 h[..][16][2],
 *             _mv8 h[..][64][2], _err32 Q[..][4], _err16 Q[..][16]: what the walk leaves in MeContext, the fields a consumer
 *             does not read under the block's flags zeroed (svtgpu.h states which); _bmv16 h[..][16][2]: tf_16x16_mv as
 *             the filter reads it (kept when the 16x16 block is split).  err32 of a use64 block is 0 here.
 *   s<k>_kinds i32[17] blocks (or positions) that: end use64 by the test, by force64, have split32 0 / 1, split16 0 / 1,
 *             skip the 16x16 search by threshold, move their best in the half / quarter / eighth stage, positions skipped
 *             by the early exit, by best == 0, ties (an evaluated position equal to a non-zero best), start MVs the clamp
 *             changes at the left / right / top / bottom.  The generator stops unless every count the set can reach is > 0.
 *   nchain, c<i>_par i32[6] {bd of the pictures, bd searched, set, mv_dist_th, tf_chroma, i}, c<i>_decay I[3], the records
 *             of the search as above with prefix c<i>, c<i>_err32p Q[2][6][4] (err32 after convert_64x64_info_to_32x32_info),
 *             c<i>_pred<r>_<p> the predictor pictures over the aligned area, c<i>_out<p> the filtered picture.
 *
 *   gen_golden_tf_search --extreme tests/golden/tf_extreme.bin    worst-case and all-tie content through the same walk,
 *   replay and SIMD second pass; the filter records are made a second time through the _avx2 planewise / central / final
 *   functions and must be equal.  The whole recipe, from the repository root after build() (REF = the reference checkout;
 *   the objects and the binary go outside the repository):
 *
 *     S=$REF/Source; C=$S/Lib/Common; E=$S/Lib/Encoder; O=/tmp/tf_search_simd; mkdir -p $O
 *     INC="-I$S/API -I$C/Codec -I$C/C_DEFAULT -I$E/Codec -I$E/C_DEFAULT -I$E/Globals -I$REF/third_party/fastfeat -I$REF \
 *       -Ioracle/_ref/enc/gen"
 *     SIMD="-O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -I$C/ASM_AVX2 -I$C/ASM_SSE2 -I$C/ASM_SSSE3 \
 *       -I$C/ASM_SSE4_1"
 *     for f in ASM_AVX2/convolve_avx2 ASM_AVX2/convolve_2d_avx2 ASM_AVX2/highbd_convolve_avx2 \
 *         ASM_AVX2/highbd_convolve_2d_avx2 ASM_SSSE3/highbd_convolve_ssse3 ASM_SSSE3/highbd_convolve_2d_ssse3 \
 *         ASM_SSE2/EbPictureOperators_Intrinsic_SSE2; do gcc $SIMD -c $C/$f.c -o $O/$(basename $f).o; done
 *     for f in ASM_AVX2/variance_avx2 ASM_AVX2/highbd_variance_avx2 ASM_SSE2/variance_sse2 \
 *         ASM_AVX2/EbTemporalFiltering_AVX2; do
 *       gcc $SIMD -I$E/ASM_AVX2 -I$E/ASM_SSE2 -c $E/$f.c -o $O/$(basename $f).o; done
 *     gcc -O2 -w -std=gnu99 -ffunction-sections $INC -Ioracle/ref_harness tests/golden/gen_golden_tf_search.c $O/*.o \
 *       -o /tmp/gen_golden_tf_search -Wl,--gc-sections -Loracle/_ref/enc -lsvtenc -Wl,-rpath,$PWD/oracle/_ref/enc -lm -lpthread
 *     /tmp/gen_golden_tf_search tests/golden/tf_search.bin
 *     /tmp/gen_golden_tf_search --extreme tests/golden/tf_extreme.bin
 *
 *   (EbTemporalFiltering_AVX2.c is needed by --extreme alone; tf_search.bin is the same with or without it.)  The file
 *   regenerates byte-identically; tests/tf_extreme_cases.py rebuilds the inputs.  The same geometry; every plane from a
 *   formula of the plane's own picture coordinates (x, y) (chroma: the same formula at half size), maxv = 2^bd - 1:
 *     content 0 max_zero    centre maxv; reference 0 all 0, reference 1 all maxv (the all-equal twin)
 *             1 checker     centre (x + y) & 1 ? maxv : 0; the references its inverse
 *             2 flat_ref    centre the drawn pictures' (above); the references 100 * sc everywhere
 *             3 v_stripes   s(u) = ((u + 800) >> 2) & 1 ? maxv : 0; centre s(x), references s(x + 3)
 *             4 h_stripes   centre s(y), references s(y + 3)
 *             5 checker2    cells of 2 x 2: centre (((x + 800) >> 1) + ((y + 800) >> 1)) & 1 ? maxv : 0; references its inverse
 *             6 near_max    centre maxv - (x & 1); the references all 0
 *     full-pel MVs 0, but flat_ref's: level lvl (0: 64x64 .. 3: 8x8), index i, block b, reference r: ((i + b + r) % 5 - 2,
 *     (i + 2 * b + lvl) % 3 - 1).
 *   Records: nset; s<k>_* as above with s<k>_par[10] the class and [11] the content, at 8 and at 10 bits each:
 *     class 0 max_zero            content 0, modes (1, 1, 1): sum^2 beyond 2^32 with variance 0, everything split to 8x8
 *           1 inv_checker_pinned  content 1, modes (0, 0, 0): the start alone; 32x32 error 66 585 600 / 66 977 856
 *           2 inv_checker_walk    content 5, eight rows over modes (1,1,1) / (2,2,2), use_2tap, sub_sampling_shift and
 *                                 enable_8x8_pred (every pair of values of two switches occurs).  Content 1 was tried first:
 *                                 no convolve form leaves the sample range on it, so no clip acts
 *           3 flat_ref            content 2: all 25 positions tie on a non-zero best, the start stays
 *           4 v_stripes, 5 h_stripes   contents 3, 4: positions that differ along the stripes tie
 *           6 th32_wide           class 1 with pred_error_32x32_th = 2^32
 *           7 near_max            content 6, modes (0, 0, 0): the 64x64 error decides use64.  At 10 bits the 64x64 sse is
 *                                 4 282 394 624, in (2^31, 2^32), the sum 4 188 160, the error 64 against 4 x 16 for the 32x32
 *                                 blocks: 64 * 14 < 64 * 16, so every block ends on the 64x64 path (checked)
 *     The generator stops unless each set reaches its point (max_zero: all split, positions skipped by best == 0; pinned:
 *     the stated errors and no split in the 32x32 blocks at x <= 96, y <= 32 -- further out the MV clamp moves the zero MV
 *     of blocks that start more than 3 samples past the picture by whole samples, an odd move gives error 0, and parents
 *     split; walk, stripes: the best moves; flat, stripes: ties; th32_wide: all 48 16x16 searches skipped).
 *     nchain = 2, c<i>_* as above plus c<i>_force64: max_zero at 8 bits and the first row of inv_checker_walk at 10 bits
 *     (searched at 10), tf_chroma 1, blocks (reference 0, 1) and (reference 1, 4) forced to the 64x64 path.
 *     nfilter = 3, x<i>_par i32[6] {bd, w, h, n_refs, mv_dist_th, i}, x<i>_decay, x<i>_split / _mv32 / _mv16 / _err32 / _err16 as
 *     gen_golden_tf.c's frame records, x<i>_out<p>, x<i>_wt H[nblk][n_refs][4][12] every quadrant's weight (count's increment;
 *     [idx_32x32][plane * 4 + quadrant]), x<i>_wide B[..] 1 where (combined >> 3) * (d_factor >> 3) passes 2^32 (from the
 *     reference's own pieces, as gen_golden_tf.c finds it), x<i>_occ i32[2][4] luma / chroma quadrants of weight 1000, of
 *     weight 0, strictly between, wide.  Predictor pictures are given over the aligned area, no search:
 *       x0 wide_frame  10 bits, 136x72, 3 predictors of a (x + y) & 1 checker centre: the centre; its inverse; the centre +
 *                      draw(0x5458000000000000 + plane, i, 601) - 300, clamped.  mv_dist_th 16.  Reference 0: zero MVs, errors
 *                      graded from 0; reference 1: MVs of 100 .. 240, d_factor >= 17 000; reference 2: MVs of +-16 383.  The
 *                      generator stops unless all four occ counts are non-zero in luma and in chroma.
 *       x1, x2 refs26  8 and 10 bits, 64x64, 26 predictors: even ones the checker centre, odd ones its inverse, zero MVs and
 *                      errors: 13 weights of 1000 and 13 of 0 in every quadrant (checked), count 14 000.
 *   Before the records the mode checks OD_DIVU_SMALL(x, d) == x / d for d = 1000 .. 1023 and every x <= d * 1023 + d / 2.
 *   No input had to be left out: the reference's C took every one, and its AVX2 forms agree on all of them.
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
void init_fn_ptr(void);
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
static void bind_convolve(int pass) {
    svt_av1_convolve_2d_copy_sr = pass ? svt_av1_convolve_2d_copy_sr_avx2 : svt_av1_convolve_2d_copy_sr_c;
    svt_av1_convolve_x_sr       = pass ? svt_av1_convolve_x_sr_avx2 : svt_av1_convolve_x_sr_c;
    svt_av1_convolve_y_sr       = pass ? svt_av1_convolve_y_sr_avx2 : svt_av1_convolve_y_sr_c;
    svt_av1_convolve_2d_sr      = pass ? svt_av1_convolve_2d_sr_avx2 : svt_av1_convolve_2d_sr_c;
    svt_av1_highbd_convolve_2d_copy_sr = pass ? svt_av1_highbd_convolve_2d_copy_sr_avx2 : svt_av1_highbd_convolve_2d_copy_sr_c;
    svt_av1_highbd_convolve_x_sr  = pass ? svt_av1_highbd_convolve_x_sr_avx2 : svt_av1_highbd_convolve_x_sr_c;
    svt_av1_highbd_convolve_y_sr  = pass ? svt_av1_highbd_convolve_y_sr_avx2 : svt_av1_highbd_convolve_y_sr_c;
    svt_av1_highbd_convolve_2d_sr = pass ? svt_av1_highbd_convolve_2d_sr_avx2 : svt_av1_highbd_convolve_2d_sr_c;
    svt_aom_asm_set_convolve_asm_table();
    svt_aom_asm_set_convolve_hbd_asm_table();
}

#define PAD 80
/* the picture: the fixture's sizes; --time sets its own */
static int W = 136, H = 72, AW = 192, AH = 128, NR = 2, NBLK = 6, BCOLS = 3, RS = 296, RH = 232;
static int g_time; /* --time: the searches alone, no replay */
static void set_size(int w, int h, int nr) {
    W = w, H = h, NR = nr, AW = (w + 63) & ~63, AH = (h + 63) & ~63, BCOLS = AW / 64, NBLK = BCOLS * (AH / 64);
    RS = W + 2 * PAD, RH = H + 2 * PAD;
}
#define HU 736
#define HV 608
#define NK 17

static int      g_simd;
static uint32_t draw(uint64_t seed, uint64_t i, uint32_t mod) {
    Rng r = {seed + i * 0x9E3779B97F4A7C15ull};
    return (uint32_t)(rng_next(&r) % mod);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

static GoldenFile *g_file;
static const char *nm(const char *pre, int i, const char *suf) {
    static char s[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(s[k], sizeof s[k], "%s%d_%s", pre, i, suf);
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

/* ---- the variance log ---- */
static AomVarianceFnPtr g_orig[BlockSizeS_ALL];
static uint32_t         g_log[1 << 16];
static int              g_nlog, g_cur;
#define WRAP(bs)                                                                                              \
    static unsigned int vf_##bs(const uint8_t *a, int as, const uint8_t *b, int bs_, unsigned int *sse) {     \
        const unsigned int v = g_orig[bs].vf(a, as, b, bs_, sse);                                             \
        return g_time ? v : (g_log[g_nlog++] = v);                                                            \
    }                                                                                                         \
    static unsigned int vfh_##bs(const uint8_t *a, int as, const uint8_t *b, int bs_, unsigned int *sse) {    \
        const unsigned int v = g_orig[bs].vf_hbd_10(a, as, b, bs_, sse);                                      \
        return g_time ? v : (g_log[g_nlog++] = v);                                                            \
    }
WRAP(BLOCK_64X64) WRAP(BLOCK_64X32) WRAP(BLOCK_32X32) WRAP(BLOCK_32X16) WRAP(BLOCK_16X16) WRAP(BLOCK_16X8) WRAP(BLOCK_8X8)
WRAP(BLOCK_8X4)
#define BIND(bs) svt_aom_mefn_ptr[bs].vf = vf_##bs, svt_aom_mefn_ptr[bs].vf_hbd_10 = vfh_##bs
/* the reference's SIMD variance functions as its RTCD picks them with AVX2 and no AVX-512 (aom_dsp_rtcd.c:331-370): _avx2
 * but for the 8-bit 8x8 / 8x4, which have an _sse2 form only, and the highbd 8x4, which has the C form only */
#define VAR_FN(n) unsigned int n(const uint8_t *, int, const uint8_t *, int, unsigned int *)
VAR_FN(svt_aom_variance64x64_avx2); VAR_FN(svt_aom_variance64x32_avx2); VAR_FN(svt_aom_variance32x32_avx2);
VAR_FN(svt_aom_variance32x16_avx2); VAR_FN(svt_aom_variance16x16_avx2); VAR_FN(svt_aom_variance16x8_avx2);
VAR_FN(svt_aom_variance8x8_sse2); VAR_FN(svt_aom_variance8x4_sse2);
VAR_FN(svt_aom_highbd_10_variance64x64_avx2); VAR_FN(svt_aom_highbd_10_variance64x32_avx2);
VAR_FN(svt_aom_highbd_10_variance32x32_avx2); VAR_FN(svt_aom_highbd_10_variance32x16_avx2);
VAR_FN(svt_aom_highbd_10_variance16x16_avx2); VAR_FN(svt_aom_highbd_10_variance16x8_avx2);
VAR_FN(svt_aom_highbd_10_variance8x8_avx2);
static AomVarianceFnPtr g_c_fn[BlockSizeS_ALL]; /* the table as init_fn_ptr leaves it on the C functions */
/* what the log wrappers call: pass 0 the _c functions, pass 1 the SIMD ones */
static void bind_variance(int pass) {
    memcpy(g_orig, g_c_fn, sizeof g_orig);
    if (!pass) return;
    g_orig[BLOCK_64X64].vf = svt_aom_variance64x64_avx2, g_orig[BLOCK_64X32].vf = svt_aom_variance64x32_avx2;
    g_orig[BLOCK_32X32].vf = svt_aom_variance32x32_avx2, g_orig[BLOCK_32X16].vf = svt_aom_variance32x16_avx2;
    g_orig[BLOCK_16X16].vf = svt_aom_variance16x16_avx2, g_orig[BLOCK_16X8].vf = svt_aom_variance16x8_avx2;
    g_orig[BLOCK_8X8].vf = svt_aom_variance8x8_sse2, g_orig[BLOCK_8X4].vf = svt_aom_variance8x4_sse2;
    g_orig[BLOCK_64X64].vf_hbd_10 = svt_aom_highbd_10_variance64x64_avx2, g_orig[BLOCK_64X32].vf_hbd_10 = svt_aom_highbd_10_variance64x32_avx2;
    g_orig[BLOCK_32X32].vf_hbd_10 = svt_aom_highbd_10_variance32x32_avx2, g_orig[BLOCK_32X16].vf_hbd_10 = svt_aom_highbd_10_variance32x16_avx2;
    g_orig[BLOCK_16X16].vf_hbd_10 = svt_aom_highbd_10_variance16x16_avx2, g_orig[BLOCK_16X8].vf_hbd_10 = svt_aom_highbd_10_variance16x8_avx2;
    g_orig[BLOCK_8X8].vf_hbd_10 = svt_aom_highbd_10_variance8x8_avx2;
}
static void wrap_variance(void) {
    init_fn_ptr();
    memcpy(g_c_fn, svt_aom_mefn_ptr, sizeof g_c_fn);
    bind_variance(0);
    BIND(BLOCK_64X64), BIND(BLOCK_64X32), BIND(BLOCK_32X32), BIND(BLOCK_32X16), BIND(BLOCK_16X16), BIND(BLOCK_16X8);
    BIND(BLOCK_8X8), BIND(BLOCK_8X4);
}

/* ---- pictures ---- */
typedef struct Pics {
    int       bd;
    uint16_t *tex;                     /* H */
    uint16_t *cen[3];                  /* aligned area, strides AW, AW / 2 */
    uint8_t  *cen8[3];
    uint16_t *ref[8][3];               /* padded, strides RS, RS / 2 */
    uint8_t  *ref8[8][3];
    int16_t   cell[2][13 * 10][2];     /* the fixture: (dx, dy) for the full-pel draw */
    int16_t (*fp64)[2], (*fp32)[4][2], (*fp16)[16][2], (*fp8)[64][2]; /* [NR * NBLK] */
} Pics;
static void alloc_fullpel(Pics *p) {
    const size_t n = (size_t)NR * NBLK;
    p->fp64 = calloc(n, sizeof *p->fp64), p->fp32 = calloc(n, sizeof *p->fp32);
    p->fp16 = calloc(n, sizeof *p->fp16), p->fp8 = calloc(n, sizeof *p->fp8);
}

static void make_pics(Pics *p, int bd, int low8) { /* low8: the 8-bit planes are the 10-bit ones >> 2 */
    const int      sc = 1 << (bd - 8), maxv = (1 << bd) - 1;
    const uint64_t S = 0x5453000000000000ull + 16 * (bd > 8);
    p->bd  = bd;
    alloc_fullpel(p);
    p->tex = malloc(sizeof(uint16_t) * HU * HV);
    for (int v = 0; v < HV; v++)
        for (int u = 0; u < HU; u++)
            p->tex[v * HU + u] = (uint16_t)clampi((u + v) * sc / 8 + (int)draw(S, (uint64_t)(v >> 3) * 92 + (u >> 3), 128 * sc) +
                                                      (int)draw(S + 1, (uint64_t)v * HU + u, 16 * sc), 0, maxv);
    for (int k = 0; k < 3; k++) {
        const int ss = k > 0, cw = AW >> ss, ch = AH >> ss, rs = RS >> ss, rh = RH >> ss;
        p->cen[k] = malloc(sizeof(uint16_t) * cw * ch), p->cen8[k] = malloc((size_t)cw * ch);
        for (int y = 0; y < ch; y++)
            for (int x = 0; x < cw; x++) {
                int v = k == 0 ? p->tex[(2 * (y + PAD) + 16) * HU + 2 * (x + PAD) + 16]
                               : clampi((int)draw(S + 8 + k, (uint64_t)y * cw + x, 64 * sc) + (2 * x + y) * sc / 4, 0, maxv);
                p->cen[k][y * cw + x] = (uint16_t)v, p->cen8[k][y * cw + x] = (uint8_t)(low8 ? v >> 2 : v);
            }
        for (int r = 0; r < NR; r++) {
            p->ref[r][k] = malloc(sizeof(uint16_t) * rs * rh), p->ref8[r][k] = malloc((size_t)rs * rh);
            for (int y = 0; y < rh; y++)
                for (int x = 0; x < rs; x++) {
                    int v;
                    if (k == 0) {
                        const int cx = x / 24, cy = y / 24, cell = cy * 13 + cx, px = x - PAD, py = y - PAD;
                        int       dx = (int)draw(S + 2 + r, 4 * cell, 13) - 6, dy = (int)draw(S + 2 + r, 4 * cell + 1, 13) - 6;
                        int       amp = (int[]){0, 2, 8, 24}[draw(S + 2 + r, 4 * cell + 2, 4)] * sc;
                        const int flat = px >= 40 && px < 88 && py >= -32 && py < 40;
                        if (cx == 3 && cy == 3) dx = 2, dy = 2, amp = 0;
                        if (cx >= 5 && cy >= 5) dx = 2, dy = 0, amp = 2 * sc;
                        if (flat) dx = dy = 0;
                        p->cell[r][cell][0] = (int16_t)dx, p->cell[r][cell][1] = (int16_t)dy;
                        v = p->tex[(2 * y + 16 + dy) * HU + 2 * x + 16 + dx];
                        if (amp) v += (int)draw(S + 4 + r, (uint64_t)y * RS + x, 2 * amp + 1) - amp;
                        if (flat) v = 100 * sc;
                    } else {
                        v = (int)draw(S + 10 + 2 * r + k, (uint64_t)y * rs + x, 64 * sc) + (2 * (x - 40) + (y - 40) + 160) * sc / 4;
                    }
                    v                      = clampi(v, 0, maxv);
                    p->ref[r][k][y * rs + x] = (uint16_t)v, p->ref8[r][k][y * rs + x] = (uint8_t)(low8 ? v >> 2 : v);
                }
        }
    }
    /* full-pel MVs: floor(d / 2) of the cell under the block's centre, +-1 on a quarter of the draws each, and one
     * component in sixteen far outside the picture so that the MV clamp acts */
    Rng rng = {S + 7};
    for (int r = 0; r < NR; r++)
        for (int b = 0; b < NBLK; b++) {
            const int bx = (b % BCOLS) * 64, by = (b / BCOLS) * 64;
            for (int lvl = 0; lvl < 4; lvl++) {
                const int n = 1 << (2 * lvl), sz = 64 >> lvl;
                for (int i = 0; i < n; i++) {
                    int x = 0, y = 0; /* nested raster index -> origin */
                    for (int l = 0; l < lvl; l++) {
                        const int q = (i >> (2 * (lvl - 1 - l))) & 3;
                        x += (q & 1) * (32 >> l), y += (q >> 1) * (32 >> l);
                    }
                    const int cxp = clampi(bx + x + sz / 2 + PAD, 0, RS - 1) / 24, cyp = clampi(by + y + sz / 2 + PAD, 0, RH - 1) / 24;
                    int16_t   mv[2];
                    for (int c = 0; c < 2; c++) {
                        const int d = p->cell[r][cyp * 13 + cxp][c];
                        int       j = (int)rng_below(&rng, 4), far = !rng_below(&rng, 16);
                        /* exact starts where the content allows an exact or a whole-block match */
                        if ((lvl <= 1 && by >= 64) || (lvl >= 2 && bx + x < 16 && by + y < 16)) j = 0, far = 0;
                        const int sgn = rng_below(&rng, 2) ? 1 : -1, mag = 150 + (int)rng_below(&rng, 50);
                        mv[c] = (int16_t)(far ? sgn * mag : -((d + 26) / 2 - 13) + (j == 2) - (j == 3));
                    }
                    const int rb = r * NBLK + b;
                    int16_t  *dst = lvl == 0 ? p->fp64[rb] : lvl == 1 ? p->fp32[rb][i] : lvl == 2 ? p->fp16[rb][i] : p->fp8[rb][i];
                    dst[0] = mv[0], dst[1] = mv[1];
                }
            }
        }
}

/* ---- the reference's state ---- */
static SequenceControlSet      *g_scs;
static PictureParentControlSet *g_pcs, *g_pcs_ref;
static void                     setup_reference(void) {
    svt_aom_setup_common_rtcd_internal(0);
    svt_aom_setup_rtcd_internal(0);
    svt_aom_asm_set_convolve_asm_table();
    svt_aom_asm_set_convolve_hbd_asm_table();
    svt_aom_build_blk_geom(GEOM_0);
    wrap_variance();
    g_scs = calloc(1, sizeof *g_scs), g_pcs = calloc(1, sizeof *g_pcs), g_pcs_ref = calloc(1, sizeof *g_pcs_ref);
    g_pcs->scs = g_scs, g_pcs->av1_cm = calloc(1, sizeof(Av1Common));
    g_scs->seq_header.sb_size = BLOCK_64X64;
    svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, W, H, W, H);
    g_pcs->av1_cm->mi_rows = H / 4, g_pcs->av1_cm->mi_cols = W / 4;
}

typedef struct Set {
    int      mode[3], use_2tap, shift, enable8, early_th;
    uint64_t th32;
    uint8_t  force64[2][6]; /* the fixture's [NR][NBLK] */
} Set;
typedef struct Out { /* one (reference, block) */
    uint8_t  use64, split32[4], split16[16];
    int16_t  mv64[2], mv32[4][2], mv16[16][2], mv8[64][2], bmv16[16][2];
    uint64_t err32[4], err16[16], err32p[4];
} Out;

/* replays one tf_subpel_search from the log; checks it against what the reference left */
static void replay(const Set *s, int b, int hbd, int px, int py, int sx, int sy, uint64_t want, int wx, int wy, int32_t *kinds,
                   uint64_t *errs, int *nerr) {
    uint64_t best = INT_MAX;
    int      bx = (int16_t)(sx * 8), by = (int16_t)(sy * 8);
    const int org[2] = {px, py}, dim[2] = {W, H}, st[2] = {bx, by};
    for (int c = 0; c < 2; c++) { /* the clamp on the start MV */
        const int q = (int16_t)(st[c] * 2), lo = -org[c] * 16 - ((4 + b) << 4), hi = (dim[c] - b - org[c]) * 16 + ((4 + b) << 4) - 16;
        kinds[13 + 2 * c] += q < lo, kinds[14 + 2 * c] += q > hi;
    }
    for (int stage = -1; stage < 3; stage++) {
        const int md = stage < 0 ? 1 : s->mode[stage], step = stage < 0 ? 0 : 4 >> stage, cx = bx, cy = by;
        int       moved = 0;
        if (!md) continue;
        for (int i = -1; i <= 1; i++)
            for (int j = -1; j <= 1; j++) {
                if (stage < 0 ? (i || j) : (!i && !j)) continue;
                if (md >= 2 && i && j) continue;
                if (best == 0) {
                    kinds[11]++;
                    continue;
                }
                if (s->early_th && best < (uint64_t)(((uint32_t)(b * b) * (uint32_t)s->early_th) << hbd)) {
                    kinds[10]++;
                    continue;
                }
                if (g_cur >= g_nlog) fprintf(stderr, "replay: the log is short\n"), exit(3);
                const uint64_t d = (uint64_t)(g_log[g_cur++] << s->shift);
                if (d == best && best) kinds[12]++;
                if (d < best) best = d, bx = (int16_t)(cx + i * step), by = (int16_t)(cy + j * step), moved = stage >= 0;
            }
        if (stage >= 0) kinds[7 + stage] += moved;
    }
    if (best != want || bx != wx || by != wy) fprintf(stderr, "replay: %dx%d block at (%d, %d) ends elsewhere\n", b, b, px, py), exit(3);
    if (errs && b == 8) errs[(*nerr)++] = best; /* the 8x8 errors: set 5 takes its threshold from them */
}

/* the walk of produce_temporally_filtered_pic for one (reference, block), :3087-3261; bd: of the pictures, sbd: searched */
static void walk(Pics *p, const Set *s, int bd, int sbd, int r, int blk, MeContext *ctx, uint8_t **pred8, uint16_t **pred16,
                 Out *o, int32_t *kinds, uint64_t *e32log, int *ne32, uint64_t *pplog, int *npp) {
    const int bc = blk % BCOLS, br = blk / BCOLS, sbx = bc * 64, sby = br * 64, hbd = sbd > 8, yoff = sbx + sby * AW;
    const int coff = bc * 32 + br * 32 * (AW / 2);
    uint32_t  stride[3] = {AW, AW / 2, AW / 2}, stride_pred[3] = {BW, BW / 2, BW / 2};
    uint8_t  *s8[3] = {p->cen8[0] + yoff, p->cen8[1] + coff, p->cen8[2] + coff};
    uint16_t *s16[3] = {p->cen[0] + yoff, p->cen[1] + coff, p->cen[2] + coff};
    EbPictureBufferDesc desc;
    uint32_t            mv64 = 0, mv32[4], mv16[16], mv8[64];
    memset(&desc, 0, sizeof desc);
    desc.buffer_y = p->ref8[r][0], desc.buffer_cb = p->ref8[r][1], desc.buffer_cr = p->ref8[r][2];
    desc.org_x = PAD, desc.org_y = PAD, desc.width = W, desc.height = H;
    desc.stride_y = RS, desc.stride_cb = RS / 2, desc.stride_cr = RS / 2;
    for (int k = 0; k < 3; k++) g_pcs_ref->altref_buffer_highbd[k] = p->ref[r][k];
    g_pcs->tf_ctrls.half_pel_mode = s->mode[0], g_pcs->tf_ctrls.quarter_pel_mode = s->mode[1];
    g_pcs->tf_ctrls.eight_pel_mode = s->mode[2], g_pcs->tf_ctrls.use_2tap = s->use_2tap;
    g_pcs->tf_ctrls.sub_sampling_shift = s->shift, g_pcs->tf_ctrls.enable_8x8_pred = s->enable8;
    g_pcs->tf_ctrls.pred_error_32x32_th = s->th32, g_pcs->tf_ctrls.subpel_early_exit_th = s->early_th;
    ctx->tf_ctrls = g_pcs->tf_ctrls, ctx->tf_subpel_early_exit_th = s->early_th, ctx->tf_use_pred_64x64_only_th = 0;
    ctx->tf_chroma = 1;
#define PACK(m) (((uint32_t)(uint16_t)(m)[1] << 16) | (uint16_t)(m)[0])
    mv64 = PACK(p->fp64[r * NBLK + blk]);
    for (int i = 0; i < 4; i++) mv32[i] = PACK(p->fp32[r * NBLK + blk][i]);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            mv16[tab16x16[idx_32x32_to_idx_16x16[i][j]]] = PACK(p->fp16[r * NBLK + blk][4 * i + j]);
            for (int k = 0; k < 4; k++) mv8[tab8x8[idx_32x32_to_idx_8x8[i][j][k]]] = PACK(p->fp8[r * NBLK + blk][16 * i + 4 * j + k]);
        }
    ctx->p_best_mv64x64 = &mv64, ctx->p_best_mv32x32 = mv32, ctx->p_best_mv16x16 = mv16, ctx->p_best_mv8x8 = mv8;
    memset(o, 0, sizeof *o);
    g_nlog = g_cur = 0;
    tf_64x64_sub_pel_search(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, stride_pred, s8, s16, stride, sbx, sby, 1, sbd);
    if (!g_time) replay(s, 64, hbd, sbx, sby, p->fp64[r * NBLK + blk][0], p->fp64[r * NBLK + blk][1], ctx->tf_64x64_block_error, ctx->tf_64x64_mv_x,
           ctx->tf_64x64_mv_y, kinds, pplog, npp);
    int use64 = g_time ? 0 : s->force64[r][blk];
    if (use64) kinds[1]++;
    if (!use64) {
        for (int i = 0; i < 4; i++) {
            ctx->idx_32x32 = i;
            tf_32x32_sub_pel_search(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, stride_pred, s8, s16, stride, sbx, sby, 1, sbd);
            if (!g_time) replay(s, 32, hbd, sbx + (i & 1) * 32, sby + (i >> 1) * 32, p->fp32[r * NBLK + blk][i][0], p->fp32[r * NBLK + blk][i][1],
                   ctx->tf_32x32_block_error[i], ctx->tf_32x32_mv_x[i], ctx->tf_32x32_mv_y[i], kinds, pplog, npp);
            if (e32log) e32log[(*ne32)++] = ctx->tf_32x32_block_error[i];
        }
        const uint64_t sum = ctx->tf_32x32_block_error[0] + ctx->tf_32x32_block_error[1] + ctx->tf_32x32_block_error[2] +
            ctx->tf_32x32_block_error[3];
        if ((ctx->tf_64x64_block_error * 14 < sum * 16) && ctx->tf_64x64_block_error < (1 << 18)) use64 = 1, kinds[0]++;
    }
    if (use64 && g_time) {
        o->use64 = 1;
        return;
    }
    if (use64) {
        tf_64x64_inter_prediction(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, sbx, sby, 1, bd);
        convert_64x64_info_to_32x32_info(g_pcs, ctx, pred8, pred16, stride_pred, s8, s16, stride, bd > 8);
        o->use64 = 1, o->mv64[0] = ctx->tf_64x64_mv_x, o->mv64[1] = ctx->tf_64x64_mv_y;
        for (int i = 0; i < 4; i++) o->mv32[i][0] = o->mv64[0], o->mv32[i][1] = o->mv64[1], o->err32p[i] = ctx->tf_32x32_block_error[i];
        return; /* mv32 here is the block record's; the motion record's is 0 (the readers say so) */
    }
    for (int i = 0; i < 4; i++) {
        ctx->idx_32x32 = i;
        if (ctx->tf_32x32_block_error[i] < g_pcs->tf_ctrls.pred_error_32x32_th) {
            ctx->tf_32x32_block_split_flag[i] = 0;
            memset(&ctx->tf_16x16_block_split_flag[i][0], 0, sizeof(ctx->tf_16x16_block_split_flag[i][0]) * 4);
            kinds[6]++;
        } else {
            tf_16x16_sub_pel_search(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, stride_pred, s8, s16, stride, sbx, sby, 1, sbd);
            for (int j = 0; j < 4; j++)
                if (!g_time) replay(s, 16, hbd, sbx + (i & 1) * 32 + (j & 1) * 16, sby + (i >> 1) * 32 + (j >> 1) * 16, p->fp16[r * NBLK + blk][4 * i + j][0],
                       p->fp16[r * NBLK + blk][4 * i + j][1], ctx->tf_16x16_block_error[4 * i + j], ctx->tf_16x16_mv_x[4 * i + j],
                       ctx->tf_16x16_mv_y[4 * i + j], kinds, pplog, npp);
            if (ctx->tf_ctrls.enable_8x8_pred) {
                tf_8x8_sub_pel_search(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, stride_pred, s8, s16, stride, sbx, sby, 1, sbd);
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 4; k++) {
                        const int q = 16 * i + 4 * j + k;
                        if (!g_time) replay(s, 8, hbd, sbx + (i & 1) * 32 + (j & 1) * 16 + (k & 1) * 8, sby + (i >> 1) * 32 + (j >> 1) * 16 + (k >> 1) * 8,
                               p->fp8[r * NBLK + blk][q][0], p->fp8[r * NBLK + blk][q][1], ctx->tf_8x8_block_error[q], ctx->tf_8x8_mv_x[q],
                               ctx->tf_8x8_mv_y[q], kinds, pplog, npp);
                    }
            }
            derive_tf_32x32_block_split_flag(ctx);
        }
        if (!g_time) tf_32x32_inter_prediction(g_pcs, ctx, g_pcs_ref, &desc, pred8, pred16, sbx, sby, 1, bd);
        const int sp = ctx->tf_32x32_block_split_flag[i];
        kinds[2 + sp]++;
        o->split32[i] = (uint8_t)sp;
        if (!sp) {
            o->mv32[i][0] = ctx->tf_32x32_mv_x[i], o->mv32[i][1] = ctx->tf_32x32_mv_y[i];
            o->err32[i] = o->err32p[i] = ctx->tf_32x32_block_error[i];
            continue;
        }
        for (int j = 0; j < 4; j++) {
            const int q = 4 * i + j, s16f = ctx->tf_16x16_block_split_flag[i][j];
            kinds[4 + s16f]++;
            o->split16[q] = (uint8_t)s16f, o->err16[q] = ctx->tf_16x16_block_error[q];
            o->bmv16[q][0] = ctx->tf_16x16_mv_x[q], o->bmv16[q][1] = ctx->tf_16x16_mv_y[q];
            if (!s16f) o->mv16[q][0] = o->bmv16[q][0], o->mv16[q][1] = o->bmv16[q][1];
            for (int k = 0; s16f && k < 4; k++) o->mv8[4 * q + k][0] = ctx->tf_8x8_mv_x[4 * q + k], o->mv8[4 * q + k][1] = ctx->tf_8x8_mv_y[4 * q + k];
        }
    }
}

/* one picture: every (block, reference) walked; with `filt` the predictors are kept and the picture is filtered */
static void run_picture(Pics *p, const Set *s, int bd, int sbd, Out *out, int32_t *kinds, uint64_t *e32log, int *ne32,
                        uint64_t *pplog, int *npp, uint16_t *predpic[][3], uint16_t *filt[3], const uint32_t *decay) {
    DECLARE_ALIGNED(32, uint32_t, accumulator[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, counter[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, pr16[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint8_t, pr8[BLK_PELS * COLOR_CHANNELS]);
    uint32_t *accum[3] = {accumulator, accumulator + BLK_PELS, accumulator + 2 * BLK_PELS};
    uint16_t *count[3] = {counter, counter + BLK_PELS, counter + 2 * BLK_PELS};
    uint16_t *pred16[3] = {pr16, pr16 + BLK_PELS, pr16 + 2 * BLK_PELS};
    uint8_t  *pred8[3] = {pr8, pr8 + BLK_PELS, pr8 + 2 * BLK_PELS};
    uint32_t  stride[3] = {AW, AW / 2, AW / 2}, stride_pred[3] = {BW, BW / 2, BW / 2};
    MeContext *ctx = calloc(1, sizeof *ctx);
    uint8_t   *o8[3];
    EbPictureBufferDesc cdesc;
    memset(&cdesc, 0, sizeof cdesc);
    cdesc.stride_y = AW;
    if (filt) {
        memcpy(ctx->tf_decay_factor_fp16, decay, 3 * sizeof(uint32_t));
        ctx->tf_mv_dist_th = 1080;
        for (int k = 0; k < 3; k++) {
            const size_t n = (size_t)(AW >> (k > 0)) * (AH >> (k > 0));
            o8[k] = malloc(n);
            memcpy(filt[k], p->cen[k], n * 2);
            for (size_t i = 0; i < n; i++) o8[k][i] = (uint8_t)p->cen[k][i];
        }
    }
    for (int blk = 0; blk < NBLK; blk++) {
        const int yoff = (blk % BCOLS) * 64 + (blk / BCOLS) * 64 * AW, coff = (blk % BCOLS) * 32 + (blk / BCOLS) * 32 * (AW / 2);
        uint8_t  *s8[3] = {p->cen8[0] + yoff, p->cen8[1] + coff, p->cen8[2] + coff};
        uint16_t *s16[3] = {p->cen[0] + yoff, p->cen[1] + coff, p->cen[2] + coff};
        if (filt) {
            /* the filter's 8-bit source is the picture itself: with 10-bit pictures the 16-bit path is taken */
            memset(accumulator, 0, sizeof accumulator), memset(counter, 0, sizeof counter);
            ctx->tf_chroma = 1;
            if (bd == 8)
                apply_filtering_central(ctx, &cdesc, s8, accum, count, BW, BH, 1, 1);
            else
                apply_filtering_central_highbd(ctx, &cdesc, s16, accum, count, BW, BH, 1, 1);
        }
        for (int r = 0; r < NR; r++) {
            memset(pr16, 0, sizeof pr16), memset(pr8, 0, sizeof pr8);
            walk(p, s, bd, sbd, r, blk, ctx, pred8, pred16, &out[r * NBLK + blk], kinds, e32log, ne32, pplog, npp);
            /* the variances the tf_*_inter_prediction / convert calls log after the searches are not the walk's */
            if (!g_time && (g_cur > g_nlog || (!out[r * NBLK + blk].use64 && g_cur != g_nlog)))
                fprintf(stderr, "replay: %d of %d logged variances consumed\n", g_cur, g_nlog), exit(3);
            if (!filt) continue;
            for (int k = 0; k < 3; k++) {
                const int bw = k ? 32 : 64, aw = AW >> (k > 0), off = k ? coff : yoff;
                for (int y = 0; y < bw; y++)
                    for (int x = 0; x < bw; x++) predpic[r][k][off + y * aw + x] = bd > 8 ? pred16[k][y * bw + x] : pred8[k][y * bw + x];
            }
            for (int row = 0; row < 2; row++)
                for (int col = 0; col < 2; col++) {
                    ctx->tf_block_col = col, ctx->tf_block_row = row;
                    apply_filtering_block_plane_wise(ctx, row, col, s8, s16, pred8, pred16, accum, count, stride, stride_pred, BW >> 1,
                                                     BH >> 1, 1, 1, bd);
                }
        }
        if (filt) get_final_filtered_pixels(ctx, o8, filt, accum, count, stride, yoff, coff, BW / 2, BH / 2, bd > 8);
    }
    if (filt)
        for (int k = 0; k < 3; k++) {
            const size_t n = (size_t)(AW >> (k > 0)) * (AH >> (k > 0));
            for (size_t i = 0; bd == 8 && i < n; i++) filt[k][i] = o8[k][i];
            free(o8[k]);
        }
    free(ctx);
}

static void put_outs(const char *pre, int i, const Out *o) {
    const int n = NR * NBLK;
    uint8_t  *u = malloc(n), *s32 = malloc(n * 4), *s16 = malloc(n * 16);
    int16_t  *m64 = malloc(n * 4), *m32 = malloc(n * 16), *m16 = malloc(n * 64), *m8 = malloc(n * 256), *b16 = malloc(n * 64);
    uint64_t *e32 = malloc(n * 32), *e16 = malloc(n * 128);
    for (int k = 0; k < n; k++) {
        u[k] = o[k].use64, memcpy(s32 + 4 * k, o[k].split32, 4), memcpy(s16 + 16 * k, o[k].split16, 16);
        memcpy(m64 + 2 * k, o[k].mv64, 4), memcpy(m32 + 8 * k, o[k].mv32, 16), memcpy(m16 + 32 * k, o[k].mv16, 64);
        memcpy(m8 + 128 * k, o[k].mv8, 256), memcpy(b16 + 32 * k, o[k].bmv16, 64);
        memcpy(e32 + 4 * k, o[k].err32, 32), memcpy(e16 + 16 * k, o[k].err16, 128);
    }
    put(nm(pre, i, "use64"), 'B', 2, NR, NBLK, 0, 0, u), put(nm(pre, i, "mv64"), 'h', 3, NR, NBLK, 2, 0, m64);
    put(nm(pre, i, "split32"), 'B', 3, NR, NBLK, 4, 0, s32), put(nm(pre, i, "split16"), 'B', 3, NR, NBLK, 16, 0, s16);
    put(nm(pre, i, "mv32"), 'h', 4, NR, NBLK, 4, 2, m32), put(nm(pre, i, "mv16"), 'h', 4, NR, NBLK, 16, 2, m16);
    put(nm(pre, i, "mv8"), 'h', 4, NR, NBLK, 64, 2, m8), put(nm(pre, i, "bmv16"), 'h', 4, NR, NBLK, 16, 2, b16);
    put(nm(pre, i, "err32"), 'Q', 3, NR, NBLK, 4, 0, e32), put(nm(pre, i, "err16"), 'Q', 3, NR, NBLK, 16, 0, e16);
    free(u), free(s32), free(s16), free(m64), free(m32), free(m16), free(m8), free(b16), free(e32), free(e16);
}

static int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* which counts a set's parameters can reach */
static int reachable(const Set *s, int set, int k) {
    if (k == 1) return set == 8;
    if (k == 5) return s->enable8;
    if (k == 6) return s->th32 != 0;
    if (k >= 7 && k <= 9) return s->mode[k - 7] != 0;
    if (k == 10) return s->early_th != 0;
    return 1;
}

static void run_simd_check(Pics *p, const Set *s, int bd, int sbd, const Out *want, const char *what, int i) {
    if (!g_simd) return;
    Out     again[NR * NBLK];
    int32_t kinds[NK] = {0};
    bind_convolve(1), bind_variance(1);
    run_picture(p, s, bd, sbd, again, kinds, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    bind_convolve(0), bind_variance(0);
    if (memcmp(again, want, sizeof again)) fprintf(stderr, "avx2 != c: %s %d\n", what, i), exit(3);
}

/* ---- --time: scripts/tf_search_perf.py's workloads through the reference's walk on one core ---- */
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static void time_reference(void) {
    static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
    g_time = 1;
    for (int k = 0; k < 2; k++) {
        const int bd = shapes[k][0], sc = 1 << (bd - 8), maxv = (1 << bd) - 1, nr = 6;
        set_size(shapes[k][1], shapes[k][2], nr);
        svt_av1_setup_scale_factors_for_frame(&g_scs->sf_identity, W, H, W, H);
        g_pcs->av1_cm->mi_rows = H / 4, g_pcs->av1_cm->mi_cols = W / 4;
        Pics *p = calloc(1, sizeof *p);
        Rng   rng = {0x5453000000300000ull + bd};
        /* the texture: 4x4-blocky noise plus fine noise, with room for the motion */
        const int tw = AW + 2 * PAD + 32, th = AH + 2 * PAD + 32, regs = RS / 96 + 1, nreg = regs * (RH / 96 + 1);
        uint16_t *tex = malloc(sizeof(uint16_t) * tw * th), *coarse = malloc(sizeof(uint16_t) * (tw / 4 + 1) * (th / 4 + 1));
        for (int i = 0; i < (tw / 4 + 1) * (th / 4 + 1); i++) coarse[i] = (uint16_t)rng_below(&rng, 160 * sc);
        for (int y = 0; y < th; y++)
            for (int x = 0; x < tw; x++) tex[y * tw + x] = (uint16_t)(coarse[(y / 4) * (tw / 4 + 1) + x / 4] + rng_below(&rng, 24 * sc));
        p->bd = bd, alloc_fullpel(p);
        p->cen[0] = malloc(sizeof(uint16_t) * AW * AH), p->cen8[0] = malloc((size_t)AW * AH);
        for (int y = 0; y < AH; y++)
            for (int x = 0; x < AW; x++) {
                const int v = tex[(y + PAD + 16) * tw + x + PAD + 16];
                p->cen[0][y * AW + x] = (uint16_t)v, p->cen8[0][y * AW + x] = (uint8_t)v;
            }
        for (int c = 1; c < 3; c++) p->cen[c] = p->cen[0], p->cen8[c] = p->cen8[0]; /* chroma is not read */
        int nb[4] = {0, 0, 0, 0};
        for (int r = 0; r < nr; r++) {
            int *mx = malloc(sizeof(int) * nreg), *my = malloc(sizeof(int) * nreg), *amp = malloc(sizeof(int) * nreg);
            for (int i = 0; i < nreg; i++)
                mx[i] = (int)rng_below(&rng, 7) - 3, my[i] = (int)rng_below(&rng, 7) - 3, amp[i] = (int[]){0, 2, 6, 20}[rng_below(&rng, 4)] * sc;
            p->ref[r][0] = malloc(sizeof(uint16_t) * RS * RH), p->ref8[r][0] = malloc((size_t)RS * RH);
            for (int y = 0; y < RH; y++)
                for (int x = 0; x < RS; x++) {
                    const int g = (y / 96) * regs + x / 96;
                    const int v = clampi(tex[(y + 16 + my[g]) * tw + x + 16 + mx[g]] + ((int)rng_below(&rng, 3) - 1) * amp[g], 0, maxv);
                    p->ref[r][0][y * RS + x] = (uint16_t)v, p->ref8[r][0][y * RS + x] = (uint8_t)v;
                }
            for (int c = 1; c < 3; c++) p->ref[r][c] = p->ref[r][0], p->ref8[r][c] = p->ref8[r][0];
            for (int b = 0; b < NBLK; b++)
                for (int lvl = 0; lvl < 4; lvl++)
                    for (int i = 0; i < 1 << (2 * lvl); i++) {
                        int x = 0, y = 0;
                        for (int l = 0; l < lvl; l++) {
                            const int q = (i >> (2 * (lvl - 1 - l))) & 3;
                            x += (q & 1) * (32 >> l), y += (q >> 1) * (32 >> l);
                        }
                        const int sz = 64 >> lvl, gx = clampi((b % BCOLS) * 64 + x + sz / 2 + PAD, 0, RS - 1);
                        const int gy = clampi((b / BCOLS) * 64 + y + sz / 2 + PAD, 0, RH - 1), g = (gy / 96) * regs + gx / 96;
                        const int jx = (int)rng_below(&rng, 8), jy = (int)rng_below(&rng, 8), rb = r * NBLK + b;
                        int16_t  *dst = lvl == 0 ? p->fp64[rb] : lvl == 1 ? p->fp32[rb][i] : lvl == 2 ? p->fp16[rb][i] : p->fp8[rb][i];
                        dst[0] = (int16_t)(-mx[g] + (jx == 0) - (jx == 1)), dst[1] = (int16_t)(-my[g] + (jy == 0) - (jy == 1));
                    }
            free(mx), free(my), free(amp);
        }
        Set s;
        memset(&s, 0, sizeof s);
        s.mode[0] = s.mode[1] = s.mode[2] = 1, s.enable8 = 1;
        Out    *out = calloc((size_t)NR * NBLK, sizeof *out);
        int32_t kinds[NK];
        double  ms[2] = {0, 0};
        for (int pass = 0; pass <= g_simd; pass++) {
            bind_convolve(pass), bind_variance(pass);
            double best = 1e30;
            for (int rep = 0; rep < 2; rep++) {
                const double t0 = now_ms();
                run_picture(p, &s, bd, bd, out, kinds, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
                const double t1 = now_ms();
                if (t1 - t0 < best) best = t1 - t0;
            }
            ms[pass] = best;
        }
        bind_convolve(0), bind_variance(0);
        for (int q = 0; q < NR * NBLK; q++) {
            nb[0] += out[q].use64;
            for (int i = 0; !out[q].use64 && i < 4; i++) {
                nb[1] += !out[q].split32[i];
                for (int j = 0; out[q].split32[i] && j < 4; j++) nb[2] += !out[q].split16[4 * i + j], nb[3] += 4 * out[q].split16[4 * i + j];
            }
        }
        printf("{\"workload\": \"%dx%d %d-bit, %d references\", \"search_c_ms\": %.1f, \"search_simd_ms\": %.1f, "
               "\"blocks_64_32_16_8\": [%d, %d, %d, %d], \"reps\": 2}\n", W, H, bd, nr, ms[0], ms[1], nb[0], nb[1], nb[2], nb[3]);
        fflush(stdout);
    }
}

/* ---- --extreme: tests/golden/tf_extreme.bin (the header lists the contents and the records) ---- */
enum { XK_MAX_ZERO, XK_CHECKER, XK_FLAT, XK_VSTRIPE, XK_HSTRIPE, XK_CHECKER2, XK_NEAR_MAX, XK_N };
enum { XC_MAX_ZERO, XC_PINNED, XC_WALK, XC_FLAT, XC_VSTRIPE, XC_HSTRIPE, XC_TH32, XC_NEAR_MAX };
/* sample (x, y) of a plane, in the picture's coordinates of that plane; r < 0: the centre */
static int xval(int kind, int r, int x, int y, int maxv, int sc) {
    const int u = kind == XK_VSTRIPE ? x : y;
    switch (kind) {
    case XK_MAX_ZERO: return r == 0 ? 0 : maxv;
    case XK_CHECKER: return ((x + y) & 1) == (r < 0) ? maxv : 0;
    case XK_CHECKER2: return ((((x + 800) >> 1) + ((y + 800) >> 1)) & 1) == (r < 0) ? maxv : 0;
    case XK_NEAR_MAX: return r < 0 ? maxv - (x & 1) : 0;
    case XK_FLAT: return 100 * sc;
    default: return ((u + (r < 0 ? 0 : 3) + 800) >> 2) & 1 ? maxv : 0;
    }
}
static void make_extreme(Pics *p, int bd, int kind) {
    const int sc = 1 << (bd - 8), maxv = (1 << bd) - 1;
    make_pics(p, bd, 0); /* the allocations, and flat_ref's centre */
    for (int k = 0; k < 3; k++) {
        const int ss = k > 0, cw = AW >> ss, ch = AH >> ss, rs = RS >> ss, rh = RH >> ss, pad = PAD >> ss;
        for (int y = 0; kind != XK_FLAT && y < ch; y++)
            for (int x = 0; x < cw; x++) p->cen[k][y * cw + x] = (uint16_t)xval(kind, -1, x, y, maxv, sc), p->cen8[k][y * cw + x] = (uint8_t)p->cen[k][y * cw + x];
        for (int r = 0; r < NR; r++)
            for (int y = 0; y < rh; y++)
                for (int x = 0; x < rs; x++)
                    p->ref[r][k][y * rs + x] = (uint16_t)xval(kind, r, x - pad, y - pad, maxv, sc), p->ref8[r][k][y * rs + x] = (uint8_t)p->ref[r][k][y * rs + x];
    }
    /* full-pel MVs: 0, but flat_ref's, which the walk must leave as they are */
    for (int r = 0; r < NR; r++)
        for (int b = 0; b < NBLK; b++)
            for (int lvl = 0; lvl < 4; lvl++)
                for (int i = 0; i < 1 << (2 * lvl); i++) {
                    const int rb = r * NBLK + b;
                    int16_t  *dst = lvl == 0 ? p->fp64[rb] : lvl == 1 ? p->fp32[rb][i] : lvl == 2 ? p->fp16[rb][i] : p->fp8[rb][i];
                    dst[0] = (int16_t)(kind == XK_FLAT ? (i + b + r) % 5 - 2 : 0), dst[1] = (int16_t)(kind == XK_FLAT ? (i + 2 * b + lvl) % 3 - 1 : 0);
                }
}

/* the filter half on given predictor pictures, as gen_golden_tf.c walks it; every quadrant's weight (count's increment)
 * and whether its avg_err product passes 2^32 are kept, [nblk][n_refs][idx_32x32][plane][quadrant] */
typedef struct XMeta {
    int32_t  split[4];
    int16_t  mv32[4][2], mv16[16][2];
    uint64_t err32[4], err16[16];
} XMeta;
extern __typeof__(svt_av1_apply_temporal_filter_planewise_medium_c)     svt_av1_apply_temporal_filter_planewise_medium_avx2;
extern __typeof__(svt_av1_apply_temporal_filter_planewise_medium_hbd_c) svt_av1_apply_temporal_filter_planewise_medium_hbd_avx2;
extern __typeof__(svt_aom_get_final_filtered_pixels_c)                  svt_aom_get_final_filtered_pixels_avx2;
extern __typeof__(svt_aom_apply_filtering_central_c)                    svt_aom_apply_filtering_central_avx2;
extern __typeof__(svt_aom_apply_filtering_central_highbd_c)             svt_aom_apply_filtering_central_highbd_avx2;
static void bind_filter(int pass) {
    svt_av1_apply_temporal_filter_planewise_medium = pass ? svt_av1_apply_temporal_filter_planewise_medium_avx2 : svt_av1_apply_temporal_filter_planewise_medium_c;
    svt_av1_apply_temporal_filter_planewise_medium_hbd = pass ? svt_av1_apply_temporal_filter_planewise_medium_hbd_avx2 : svt_av1_apply_temporal_filter_planewise_medium_hbd_c;
    get_final_filtered_pixels      = pass ? svt_aom_get_final_filtered_pixels_avx2 : svt_aom_get_final_filtered_pixels_c;
    apply_filtering_central        = pass ? svt_aom_apply_filtering_central_avx2 : svt_aom_apply_filtering_central_c;
    apply_filtering_central_highbd = pass ? svt_aom_apply_filtering_central_highbd_avx2 : svt_aom_apply_filtering_central_highbd_c;
}
static uint32_t xwindow(const uint16_t *s, int ss, const uint16_t *p, int ps, int hw, int bd) { /* window_error_quad_fp8 */
    uint32_t sum = 0;
    for (int y = 0; y < hw; y++)
        for (int x = 0; x < hw; x++) {
            const int df = s[y * ss + x] - p[y * ps + x];
            sum += (uint32_t)(df * df);
        }
    sum >>= 2 * (bd - 8);
    return (((sum << 4) / hw) << 4) / hw;
}
static void xfilter(int bd, int w, int h, uint16_t *cen[3], uint16_t *(*pred)[3], int nr, const XMeta *meta, const uint32_t *decay,
                    int mv_dist_th, uint16_t *out[3], uint16_t *wt, uint8_t *wide) {
    DECLARE_ALIGNED(32, uint32_t, accumulator[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, counter[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, pr16[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint8_t, pr8[BLK_PELS * COLOR_CHANNELS]);
    uint32_t *accum[3] = {accumulator, accumulator + BLK_PELS, accumulator + 2 * BLK_PELS};
    uint16_t *count[3] = {counter, counter + BLK_PELS, counter + 2 * BLK_PELS};
    uint16_t *pred16[3] = {pr16, pr16 + BLK_PELS, pr16 + 2 * BLK_PELS};
    uint8_t  *pred8[3] = {pr8, pr8 + BLK_PELS, pr8 + 2 * BLK_PELS};
    const int aw = (w + 63) & ~63, ah = (h + 63) & ~63, bcols = aw / 64, nblk = bcols * (ah / 64);
    uint32_t  stride[3] = {aw, aw / 2, aw / 2}, stride_pred[3] = {BW, BW / 2, BW / 2};
    MeContext *ctx = calloc(1, sizeof *ctx);
    uint8_t   *c8[3], *o8[3];
    EbPictureBufferDesc cdesc;
    memset(&cdesc, 0, sizeof cdesc);
    cdesc.stride_y = aw;
    memcpy(ctx->tf_decay_factor_fp16, decay, 3 * sizeof(uint32_t));
    ctx->tf_mv_dist_th = (uint16_t)mv_dist_th, ctx->tf_chroma = 1;
    const uint32_t thr = AOMMAX((ctx->tf_mv_dist_th << 16) / 10, 1 << 16);
    for (int k = 0; k < 3; k++) {
        const size_t n = (size_t)(aw >> (k > 0)) * (ah >> (k > 0));
        c8[k] = malloc(n), o8[k] = malloc(n);
        memcpy(out[k], cen[k], n * 2);
        for (size_t i = 0; i < n; i++) c8[k][i] = o8[k][i] = (uint8_t)cen[k][i];
    }
    for (int blk = 0; blk < nblk; blk++) {
        const int yoff = (blk % bcols) * 64 + (blk / bcols) * 64 * aw, coff = (blk % bcols) * 32 + (blk / bcols) * 32 * (aw / 2);
        uint8_t  *s8[3] = {c8[0] + yoff, c8[1] + coff, c8[2] + coff};
        uint16_t *s16[3] = {cen[0] + yoff, cen[1] + coff, cen[2] + coff};
        memset(accumulator, 0, sizeof accumulator), memset(counter, 0, sizeof counter);
        if (bd == 8)
            apply_filtering_central(ctx, &cdesc, s8, accum, count, BW, BH, 1, 1);
        else
            apply_filtering_central_highbd(ctx, &cdesc, s16, accum, count, BW, BH, 1, 1);
        for (int r = 0; r < nr; r++) {
            const XMeta *m = &meta[r * nblk + blk];
            for (int k = 0; k < 3; k++) {
                const int bw = k ? 32 : 64, st = aw >> (k > 0), off = k ? coff : yoff;
                for (int y = 0; y < bw; y++)
                    for (int x = 0; x < bw; x++) pred16[k][y * bw + x] = pred[r][k][off + y * st + x], pred8[k][y * bw + x] = (uint8_t)pred16[k][y * bw + x];
            }
            for (int i = 0; i < 4; i++) {
                ctx->tf_32x32_block_split_flag[i] = m->split[i], ctx->tf_32x32_block_error[i] = m->err32[i];
                ctx->tf_32x32_mv_x[i] = m->mv32[i][0], ctx->tf_32x32_mv_y[i] = m->mv32[i][1];
            }
            for (int i = 0; i < 16; i++)
                ctx->tf_16x16_mv_x[i] = m->mv16[i][0], ctx->tf_16x16_mv_y[i] = m->mv16[i][1], ctx->tf_16x16_block_error[i] = m->err16[i];
            for (int idx = 0; idx < 4; idx++) {
                const int row = idx >> 1, col = idx & 1;
                uint16_t  before[3][4];
                uint32_t  lw[4];
                uint16_t *wq = wt + (((size_t)blk * nr + r) * 4 + idx) * 12;
                uint8_t  *dq = wide + (((size_t)blk * nr + r) * 4 + idx) * 12;
                for (int k = 0; k < 3; k++)
                    for (int q = 0; q < 4; q++) {
                        const int bw = k ? 32 : 64, hw = bw / 4, o = (row * (bw / 2) + (q >> 1) * hw) * bw + col * (bw / 2) + (q & 1) * hw;
                        const int so = (row * (bw / 2) + (q >> 1) * hw) * (aw >> (k > 0)) + col * (bw / 2) + (q & 1) * hw;
                        before[k][q] = count[k][o];
                        /* the product of :1093-1098 in 64 bits, from the reference's own pieces */
                        uint32_t we = xwindow(s16[k] + so, aw >> (k > 0), pred16[k] + o, bw, hw, bd);
                        if (!k) lw[q] = we;
                        else we = (we * 5 + lw[q]) / 6;
                        const int      sp = m->split[idx], mx = sp ? m->mv16[idx * 4 + q][0] : m->mv32[idx][0];
                        const int      my = sp ? m->mv16[idx * 4 + q][1] : m->mv32[idx][1];
                        const uint32_t d = AOMMAX((sqrt_fast(((uint32_t)(mx * mx + my * my)) << 8) << 12) / (thr >> 8), 1 << 8);
                        const uint32_t be = sp ? (uint32_t)(m->err16[idx * 4 + q] >> (bd > 8 ? 4 : 0)) : (uint32_t)(m->err32[idx] >> (bd > 8 ? 6 : 2));
                        const uint64_t comb = (uint32_t)(we * 5 + be) / 6;
                        dq[k * 4 + q] = (comb >> 3) * (uint64_t)(d >> 3) >= ((uint64_t)1 << 32);
                    }
                ctx->tf_block_col = col, ctx->tf_block_row = row;
                apply_filtering_block_plane_wise(ctx, row, col, s8, s16, pred8, pred16, accum, count, stride, stride_pred, BW >> 1, BH >> 1, 1, 1, bd);
                for (int k = 0; k < 3; k++)
                    for (int q = 0; q < 4; q++) {
                        const int bw = k ? 32 : 64, hw = bw / 4, o = (row * (bw / 2) + (q >> 1) * hw) * bw + col * (bw / 2) + (q & 1) * hw;
                        wq[k * 4 + q] = (uint16_t)(count[k][o] - before[k][q]);
                    }
            }
        }
        get_final_filtered_pixels(ctx, o8, out, accum, count, stride, yoff, coff, BW / 2, BH / 2, bd > 8);
    }
    for (int k = 0; k < 3; k++) {
        const size_t n = (size_t)(aw >> (k > 0)) * (ah >> (k > 0));
        for (size_t i = 0; bd == 8 && i < n; i++) out[k][i] = o8[k][i];
        free(c8[k]), free(o8[k]);
    }
    free(ctx);
}

/* one filter record: both passes, compared; the counts of what the quadrants met into occ[2][4] (luma / chroma: weight 1000,
 * weight 0, strictly between, product beyond 2^32) */
static void put_filter(int i, int bd, int w, int h, uint16_t *cen[3], uint16_t *(*pred)[3], int nr, const XMeta *meta, const uint32_t *decay,
                       int mv_dist_th, int32_t occ[2][4]) {
    const int aw = (w + 63) & ~63, ah = (h + 63) & ~63, nblk = (aw / 64) * (ah / 64), nq = nblk * nr * 48;
    uint16_t *out[2][3], *wt[2];
    uint8_t  *wide[2];
    for (int pass = 0; pass <= g_simd; pass++) {
        for (int k = 0; k < 3; k++) out[pass][k] = calloc((size_t)(aw >> (k > 0)) * (ah >> (k > 0)), 2);
        wt[pass] = calloc(nq, 2), wide[pass] = calloc(nq, 1);
        bind_filter(pass);
        xfilter(bd, w, h, cen, pred, nr, meta, decay, mv_dist_th, out[pass], wt[pass], wide[pass]);
        bind_filter(0);
        if (pass && memcmp(wt[0], wt[1], (size_t)nq * 2)) fprintf(stderr, "avx2 != c: filter %d weights\n", i), exit(3);
        for (int k = 0; pass && k < 3; k++)
            if (memcmp(out[0][k], out[1][k], (size_t)(aw >> (k > 0)) * (ah >> (k > 0)) * 2)) fprintf(stderr, "avx2 != c: filter %d plane %d\n", i, k), exit(3);
    }
    memset(occ, 0, 8 * sizeof(int32_t));
    for (int q = 0; q < nq; q++) {
        int32_t *o = occ[(q % 12) >= 4];
        o[0] += wt[0][q] == 1000, o[1] += wt[0][q] == 0, o[2] += wt[0][q] > 0 && wt[0][q] < 1000, o[3] += wide[0][q];
    }
    int32_t   par[6] = {bd, w, h, nr, mv_dist_th, i};
    int32_t  *sp = malloc(sizeof(int32_t) * 4 * nr * nblk);
    int16_t  *m32 = malloc(sizeof(int16_t) * 8 * nr * nblk), *m16 = malloc(sizeof(int16_t) * 32 * nr * nblk);
    uint64_t *e32 = malloc(sizeof(uint64_t) * 4 * nr * nblk), *e16 = malloc(sizeof(uint64_t) * 16 * nr * nblk);
    for (int k = 0; k < nr * nblk; k++) {
        memcpy(sp + 4 * k, meta[k].split, 16), memcpy(m32 + 8 * k, meta[k].mv32, 16), memcpy(m16 + 32 * k, meta[k].mv16, 64);
        memcpy(e32 + 4 * k, meta[k].err32, 32), memcpy(e16 + 16 * k, meta[k].err16, 128);
    }
    put(nm("x", i, "par"), 'i', 1, 6, 0, 0, 0, par), put(nm("x", i, "decay"), 'I', 1, 3, 0, 0, 0, decay);
    put(nm("x", i, "split"), 'i', 3, nr, nblk, 4, 0, sp), put(nm("x", i, "mv32"), 'h', 4, nr, nblk, 4, 2, m32);
    put(nm("x", i, "mv16"), 'h', 4, nr, nblk, 16, 2, m16), put(nm("x", i, "err32"), 'Q', 3, nr, nblk, 4, 0, e32);
    put(nm("x", i, "err16"), 'Q', 3, nr, nblk, 16, 0, e16);
    put(nm("x", i, "wt"), 'H', 4, nblk, nr, 4, 12, wt[0]), put(nm("x", i, "wide"), 'B', 4, nblk, nr, 4, 12, wide[0]);
    put(nm("x", i, "occ"), 'i', 2, 2, 4, 0, 0, occ);
    for (int k = 0; k < 3; k++) {
        char suf[16];
        snprintf(suf, sizeof suf, "out%d", k);
        put_plane(nm("x", i, suf), bd, h >> (k > 0), w >> (k > 0), out[0][k], aw >> (k > 0));
    }
    fprintf(stderr, "filter %d (%d bits, %d references): luma %d %d %d %d, chroma %d %d %d %d\n", i, bd, nr, occ[0][0], occ[0][1], occ[0][2],
            occ[0][3], occ[1][0], occ[1][1], occ[1][2], occ[1][3]);
    free(sp), free(m32), free(m16), free(e32), free(e16);
    for (int pass = 0; pass <= g_simd; pass++) {
        for (int k = 0; k < 3; k++) free(out[pass][k]);
        free(wt[pass]), free(wide[pass]);
    }
}

static int extreme(const char *path) {
    GoldenFile g = golden_open(path);
    g_file       = &g;
    setup_reference();
    /* OD_DIVU_SMALL against plain division for every divisor below OD_DIVU_DMAX a count can be (1000 .. 1023: the centre
     * and references of small weight) and every accum + (count >> 1) a 10-bit picture can form with it */
    for (uint32_t d = 1000; d < 1024; d++)
        for (uint32_t x = 0; x <= d * 1023u + (d >> 1); x++)
            if (OD_DIVU_SMALL(x, d) != x / d) fprintf(stderr, "OD_DIVU_SMALL(%u, %u) differs from the quotient\n", x, d), exit(3);
    static const struct { int cls, kind; } rows[] = {{XC_MAX_ZERO, XK_MAX_ZERO}, {XC_PINNED, XK_CHECKER}, {XC_WALK, XK_CHECKER2}, {XC_FLAT, XK_FLAT},
                                                     {XC_VSTRIPE, XK_VSTRIPE}, {XC_HSTRIPE, XK_HSTRIPE}, {XC_TH32, XK_CHECKER}, {XC_NEAR_MAX, XK_NEAR_MAX}};
    static Pics pics[2][XK_N];
    for (int d = 0; d < 2; d++)
        for (int k = 0; k < XK_N; k++) make_extreme(&pics[d][k], d ? 10 : 8, k);
    int  nset = 0, chain_set[2] = {-1, -1};
    Set  chain_s[2];
    for (size_t row = 0; row < sizeof rows / sizeof rows[0]; row++)
        for (int d = 0; d < 2; d++)
            for (int v = 0; v < (rows[row].cls == XC_WALK ? 8 : 1); v++) {
                const int bd = d ? 10 : 8, cls = rows[row].cls, kind = rows[row].kind;
                Pics     *p = &pics[d][kind];
                Set       s;
                memset(&s, 0, sizeof s);
                s.mode[0] = s.mode[1] = s.mode[2] = 1, s.enable8 = 1;
                if (cls == XC_PINNED || cls == XC_TH32 || cls == XC_NEAR_MAX) s.mode[0] = s.mode[1] = s.mode[2] = 0;
                if (cls == XC_TH32) s.th32 = (uint64_t)1 << 32;
                if (cls == XC_WALK) { /* the eight rows of the orthogonal array over the four switches */
                    const int m = v & 1, t = v >> 1 & 1, sh = v >> 2 & 1;
                    s.mode[0] = s.mode[1] = s.mode[2] = 1 + m, s.use_2tap = t, s.shift = sh, s.enable8 = !(m ^ t ^ sh);
                }
                Out     out[NR * NBLK];
                int32_t kinds[NK] = {0}, par[12] = {bd, s.mode[0], s.mode[1], s.mode[2], s.use_2tap, s.shift, s.enable8, 0, NR, PAD, cls, kind};
                int     dummy = 0;
                static uint64_t pp_sink[2 * 6 * 85];
                run_picture(p, &s, bd, bd, out, kinds, NULL, NULL, pp_sink, &dummy, NULL, NULL, NULL);
                run_simd_check(p, &s, bd, bd, out, "extreme set", nset);
                /* what the content is there for */
                int n64 = 0, nsp32 = 0, nsp16 = 0, moved = 0;
                for (int k = 0; k < NR * NBLK; k++) {
                    n64 += out[k].use64;
                    for (int i = 0; i < 4; i++) nsp32 += out[k].split32[i], moved += !out[k].split32[i] && (out[k].mv32[i][0] || out[k].mv32[i][1]);
                    for (int i = 0; i < 16; i++) nsp16 += out[k].split16[i];
                }
                int ok = 1;
                if (cls == XC_MAX_ZERO) ok = !n64 && nsp32 == NR * NBLK * 4 && nsp16 == NR * NBLK * 16 && kinds[11] > 0;
                if (cls == XC_PINNED) { /* the 32x32 blocks none of whose sub-blocks the MV clamp moves: x <= 96, y <= 32 */
                    ok = !n64;
                    for (int k = 0; k < NR * NBLK; k++)
                        for (int i = 0; i < 4; i++)
                            if ((k % NBLK % BCOLS) * 64 + (i & 1) * 32 <= 96 && (k % NBLK / BCOLS) * 64 + (i >> 1) * 32 <= 32)
                                ok &= !out[k].split32[i] && out[k].err32[i] == (d ? 66977856u : 66585600u);
                }
                if (cls == XC_TH32) ok = !n64 && !nsp32 && kinds[6] == NR * NBLK * 4;
                if (cls == XC_WALK) ok = kinds[7] > 0 && moved > 0;
                if (cls == XC_NEAR_MAX) ok = n64 == NR * NBLK && kinds[0] == NR * NBLK;
                if (cls == XC_FLAT) ok = kinds[12] > 0 && !kinds[7] && !kinds[8] && !kinds[9];
                if (cls == XC_VSTRIPE || cls == XC_HSTRIPE) ok = kinds[12] > 0 && kinds[7] > 0;
                if (!ok) fprintf(stderr, "extreme set %d (class %d, %d bits) does not reach its point: %d use64, %d split32, %d split16, err32 %llu\n", nset, cls, bd, n64, nsp32, nsp16, (unsigned long long)out[0].err32[0]), exit(3);
                put(nm("s", nset, "par"), 'i', 1, 12, 0, 0, 0, par);
                put(nm("s", nset, "th32"), 'Q', 1, 1, 0, 0, 0, &s.th32);
                put(nm("s", nset, "force64"), 'B', 2, NR, NBLK, 0, 0, s.force64);
                put(nm("s", nset, "kinds"), 'i', 1, NK, 0, 0, 0, kinds);
                put_outs("s", nset, out);
                fprintf(stderr, "%2d bits class %d kind %d:", bd, cls, kind);
                for (int k = 0; k < NK; k++) fprintf(stderr, " %d", kinds[k]);
                fprintf(stderr, "\n");
                /* the chains' parameter sets: max_zero at 8 bits, the default row of the walk at 10 */
                if ((cls == XC_MAX_ZERO && !d) || (cls == XC_WALK && d && v == 0)) chain_set[d] = nset, chain_s[d] = s;
                nset++;
            }
    int32_t ns = nset;
    put("nset", 'i', 1, 1, 0, 0, 0, &ns);
    /* the chains, tf_chroma 1: one block of each reference forced to the 64x64 path */
    static const uint32_t decay[3] = {6000000, 9000000, 12000000};
    for (int c = 0; c < 2; c++) {
        const int bd = c ? 10 : 8;
        Pics     *p = &pics[c][c ? XK_CHECKER2 : XK_MAX_ZERO];
        Set      *s = &chain_s[c];
        s->force64[0][1] = s->force64[1][4] = 1;
        Out       out[NR * NBLK];
        int32_t   kinds[NK] = {0}, par[6] = {bd, bd, chain_set[c], 1080, 1, c};
        uint16_t *predpic[NR][3], *filt[3];
        uint64_t  pp_sink[NR * NBLK * 85], e32p[NR * NBLK * 4];
        int       dummy = 0;
        for (int k = 0; k < 3; k++) {
            const size_t n = (size_t)(AW >> (k > 0)) * (AH >> (k > 0));
            filt[k] = calloc(n, 2);
            for (int r = 0; r < NR; r++) predpic[r][k] = calloc(n, 2);
        }
        run_picture(p, s, bd, bd, out, kinds, NULL, NULL, pp_sink, &dummy, predpic, filt, decay);
        run_simd_check(p, s, bd, bd, out, "extreme chain", c);
        if (!out[1].use64 || !out[NBLK + 4].use64) fprintf(stderr, "extreme chain %d: no forced block\n", c), exit(3);
        for (int k = 0; k < NR * NBLK; k++) memcpy(e32p + 4 * k, out[k].err32p, 32);
        put(nm("c", c, "par"), 'i', 1, 6, 0, 0, 0, par), put(nm("c", c, "decay"), 'I', 1, 3, 0, 0, 0, decay);
        put(nm("c", c, "force64"), 'B', 2, NR, NBLK, 0, 0, s->force64);
        put_outs("c", c, out);
        put(nm("c", c, "err32p"), 'Q', 3, NR, NBLK, 4, 0, e32p);
        for (int r = 0; r < NR; r++)
            for (int k = 0; k < 3; k++) {
                char suf[16];
                snprintf(suf, sizeof suf, "pred%d_%d", r, k);
                put_plane(nm("c", c, suf), bd, AH >> (k > 0), AW >> (k > 0), predpic[r][k], AW >> (k > 0));
            }
        for (int k = 0; k < 3; k++) {
            char suf[16];
            snprintf(suf, sizeof suf, "out%d", k);
            put_plane(nm("c", c, suf), bd, H >> (k > 0), W >> (k > 0), filt[k], AW >> (k > 0));
        }
    }
    int32_t nc = 2;
    put("nchain", 'i', 1, 1, 0, 0, 0, &nc);
    /* the filter records: wide_frame, refs26 at 8 and 10 bits */
    for (int f = 0; f < 3; f++) {
        const int bd = f == 1 ? 8 : 10, w = f ? 64 : W, h = f ? 64 : H, nr = f ? 26 : 3, aw = (w + 63) & ~63, ah = (h + 63) & ~63;
        const int nblk = (aw / 64) * (ah / 64), maxv = (1 << bd) - 1, th = f ? 1080 : 16;
        uint16_t *cen[3], *(*pred)[3] = calloc(nr, sizeof *pred);
        XMeta    *meta = calloc((size_t)nr * nblk, sizeof *meta);
        for (int k = 0; k < 3; k++) {
            const int cw = aw >> (k > 0), ch = ah >> (k > 0);
            cen[k] = malloc(sizeof(uint16_t) * cw * ch);
            for (int r = 0; r < nr; r++) pred[r][k] = malloc(sizeof(uint16_t) * cw * ch);
            for (int y = 0; y < ch; y++)
                for (int x = 0; x < cw; x++) {
                    const int v = (x + y) & 1 ? maxv : 0, i = y * cw + x;
                    cen[k][i] = (uint16_t)v;
                    for (int r = 0; r < nr; r++)
                        pred[r][k][i] = (uint16_t)(f ? (r & 1 ? maxv - v : v)
                                                     : r == 0 ? v : r == 1 ? maxv - v
                                                              : clampi(v + (int)draw(0x5458000000000000ull + k, (uint64_t)i, 601) - 300, 0, maxv));
                }
        }
        /* wide_frame's metadata: reference 0 (the centre) has errors graded from 0 so that its weights run from 1000 down,
         * reference 1 (full range) MVs of 100 to 240 eighths, whose d_factor of 17 000 and more takes the product past 2^32,
         * reference 2 MVs of +-16 383, where (col^2 + row^2) << 8 wraps 32 bits */
        for (int r = 0; !f && r < nr; r++)
            for (int b = 0; b < nblk; b++) {
                XMeta *m = &meta[r * nblk + b];
                for (int i = 0; i < 4; i++) {
                    m->split[i] = (b + i + r) & 1;
                    m->err32[i] = r == 0 ? (uint64_t)((b * 4 + i) % 8) * 8000000 : r == 1 ? 1000000 : 4000000;
                    m->mv32[i][0] = (int16_t)(r == 0 ? 0 : r == 1 ? 100 + 20 * i : (i & 1 ? -16383 : 16383));
                    m->mv32[i][1] = (int16_t)(r == 0 ? 0 : r == 1 ? -(120 + 10 * b) : (b & 1 ? 16383 : -16383));
                }
                for (int i = 0; i < 16; i++) {
                    m->err16[i] = r == 0 ? (uint64_t)((b + i) % 8) * 1000000 : r == 1 ? 300000 : 1000000;
                    m->mv16[i][0] = (int16_t)(r == 0 ? 0 : r == 1 ? 110 + 8 * i : (i & 2 ? 16383 : -16383));
                    m->mv16[i][1] = (int16_t)(r == 0 ? 0 : r == 1 ? 130 - 4 * i : (i & 1 ? 16383 : -16383));
                }
            }
        int32_t occ[2][4];
        put_filter(f, bd, w, h, cen, pred, nr, meta, decay, th, occ);
        for (int c = 0; c < 2; c++)
            for (int k = 0; k < (f ? 2 : 4); k++)
                if (!occ[c][k]) fprintf(stderr, "filter %d: %s count %d is zero\n", f, c ? "chroma" : "luma", k), exit(3);
        if (f && (occ[0][0] != 13 * 16 || occ[0][1] != 13 * 16)) fprintf(stderr, "filter %d: not 13 + 13\n", f), exit(3);
        for (int k = 0; k < 3; k++) {
            free(cen[k]);
            for (int r = 0; r < nr; r++) free(pred[r][k]);
        }
        free(pred), free(meta);
    }
    int32_t nf = 3;
    put("nfilter", 'i', 1, 1, 0, 0, 0, &nf);
    golden_close(&g);
    fprintf(stderr, "%d search records, 2 chain records, 3 filter records; %s\n", nset,
            g_simd ? "every record equal with the convolve, variance and filter pointers on the SIMD functions" : "no AVX2 on this host: the _c functions only");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --extreme <out.bin> | --time\n", argv[0]);
        return 2;
    }
    g_simd = __builtin_cpu_supports("avx2") ? 1 : 0;
    if (!strcmp(argv[1], "--time")) {
        setup_reference();
        time_reference();
        return 0;
    }
    if (!strcmp(argv[1], "--extreme") && argc > 2) return extreme(argv[2]);
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    setup_reference();
    static Pics pics[2], pics10as8;
    make_pics(&pics[0], 8, 0), make_pics(&pics[1], 10, 0), make_pics(&pics10as8, 10, 1);
    int nset = 0, bad = 0;
    Set sets[2][9];
    for (int d = 0; d < 2; d++) {
        const int bd = d ? 10 : 8;
        Pics     *p = &pics[d];
        put(nm("f", bd, "mv64"), 'h', 3, NR, NBLK, 2, 0, p->fp64), put(nm("f", bd, "mv32"), 'h', 4, NR, NBLK, 4, 2, p->fp32);
        put(nm("f", bd, "mv16"), 'h', 4, NR, NBLK, 16, 2, p->fp16), put(nm("f", bd, "mv8"), 'h', 4, NR, NBLK, 64, 2, p->fp8);
        uint64_t e32log[NR * NBLK * 4], pplog[NR * NBLK * 85];
        int      ne32 = 0, npp = 0;
        for (int set = 0; set < 9; set++) {
            Set *s = &sets[d][set];
            memset(s, 0, sizeof *s);
            s->mode[0] = s->mode[1] = s->mode[2] = 1, s->enable8 = 1;
            if (set == 1) s->mode[0] = s->mode[1] = s->mode[2] = 2;
            if (set == 2) s->mode[1] = s->mode[2] = 0;
            if (set == 3) s->shift = 1;
            if (set == 4) s->use_2tap = 1;
            if (set == 5) { /* the median per-sample error of the default set's 8x8 blocks, at least 1 */
                uint64_t v[NR * NBLK * 85];
                int      n = 0;
                for (int k = 0; k < npp; k++) v[n++] = pplog[k];
                qsort(v, n, sizeof v[0], cmp_u64);
                s->early_th = clampi((int)((v[n / 2] >> d) / 64) + 1, 1, 255);
            }
            if (set == 6) {
                qsort(e32log, ne32, sizeof e32log[0], cmp_u64);
                s->th32 = e32log[ne32 / 2] + 1;
            }
            if (set == 7) s->enable8 = 0;
            if (set == 8)
                for (int k = 0; k < NR * NBLK; k++) s->force64[k / NBLK][k % NBLK] = (uint8_t)(k % 3 == 1);
            Out     out[NR * NBLK];
            int32_t kinds[NK] = {0}, par[12] = {bd, s->mode[0], s->mode[1], s->mode[2], s->use_2tap, s->shift, s->enable8,
                                                s->early_th, NR, PAD, set, 0};
            int     dummy = 0;
            static uint64_t pp_sink[2 * 6 * 85];
            /* the default set records the 32x32 errors and the 8x8 errors that sets 5 and 6 take their thresholds from */
            if (set == 0) {
                run_picture(p, s, bd, bd, out, kinds, e32log, &ne32, pplog, &npp, NULL, NULL, NULL);
            } else {
                run_picture(p, s, bd, bd, out, kinds, NULL, NULL, pp_sink, &dummy, NULL, NULL, NULL);
            }
            run_simd_check(p, s, bd, bd, out, "set", nset);
            for (int k = 0; k < NK; k++)
                if (reachable(s, set, k) && !kinds[k]) fprintf(stderr, "%d bits, set %d: count %d is zero\n", bd, set, k), bad = 1;
            put(nm("s", nset, "par"), 'i', 1, 12, 0, 0, 0, par);
            put(nm("s", nset, "th32"), 'Q', 1, 1, 0, 0, 0, &s->th32);
            put(nm("s", nset, "force64"), 'B', 2, NR, NBLK, 0, 0, s->force64);
            put(nm("s", nset, "kinds"), 'i', 1, NK, 0, 0, 0, kinds);
            put_outs("s", nset, out);
            fprintf(stderr, "%2d bits set %d (early %d, th32 %llu):", bd, set, s->early_th, (unsigned long long)s->th32);
            for (int k = 0; k < NK; k++) fprintf(stderr, " %d", kinds[k]);
            fprintf(stderr, "\n");
            nset++;
        }
    }
    if (bad) return 3; /* every zero count has been named */
    int32_t ns = nset;
    put("nset", 'i', 1, 1, 0, 0, 0, &ns);
    /* the chains: 8-bit; 10-bit pictures searched on their 8-bit planes; 8-bit with sub_sampling_shift 1 (set 3) */
    static const uint32_t decay[3] = {6000000, 9000000, 12000000};
    for (int c = 0; c < 3; c++) {
        const int bd = c == 1 ? 10 : 8, set = c == 2 ? 3 : 0;
        Pics     *p = c == 1 ? &pics10as8 : &pics[0];
        Set      *s = &sets[0][set];
        Out       out[NR * NBLK];
        int32_t   kinds[NK] = {0}, par[6] = {bd, 8, set, 1080, 1, c};
        uint16_t *predpic[NR][3], *filt[3];
        uint64_t  pp_sink[NR * NBLK * 85], e32p[NR * NBLK * 4];
        int       dummy = 0;
        for (int k = 0; k < 3; k++) {
            const size_t n = (size_t)(AW >> (k > 0)) * (AH >> (k > 0));
            filt[k] = calloc(n, 2);
            for (int r = 0; r < NR; r++) predpic[r][k] = calloc(n, 2);
        }
        run_picture(p, s, bd, 8, out, kinds, NULL, NULL, pp_sink, &dummy, predpic, filt, decay);
        run_simd_check(p, s, bd, 8, out, "chain", c);
        for (int k = 0; k < NR * NBLK; k++) memcpy(e32p + 4 * k, out[k].err32p, 32);
        put(nm("c", c, "par"), 'i', 1, 6, 0, 0, 0, par), put(nm("c", c, "decay"), 'I', 1, 3, 0, 0, 0, decay);
        put_outs("c", c, out);
        put(nm("c", c, "err32p"), 'Q', 3, NR, NBLK, 4, 0, e32p);
        for (int r = 0; r < NR; r++)
            for (int k = 0; k < 3; k++) {
                char suf[16];
                snprintf(suf, sizeof suf, "pred%d_%d", r, k);
                put_plane(nm("c", c, suf), bd, AH >> (k > 0), AW >> (k > 0), predpic[r][k], AW >> (k > 0));
            }
        for (int k = 0; k < 3; k++) {
            char suf[16];
            snprintf(suf, sizeof suf, "out%d", k);
            put_plane(nm("c", c, suf), bd, H >> (k > 0), W >> (k > 0), filt[k], AW >> (k > 0));
        }
    }
    int32_t nc = 3;
    put("nchain", 'i', 1, 1, 0, 0, 0, &nc);
    golden_close(&g);
    fprintf(stderr, "%d search records, 3 chain records; %s\n", nset,
            g_simd ? "every record equal with the convolve and variance pointers on the SIMD functions" : "no AVX2 on this host: the _c functions only");
    return 0;
}
