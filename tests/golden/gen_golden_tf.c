/*
 * gen_golden_tf.c — writes tests/golden/tf.bin: the filter half of the reference's temporal filter (EbTemporalFiltering.c:
 * svt_estimate_noise_fp16_c / _highbd_fp16_c, svt_aom_noise_log1p_fp16, apply_filtering_central(_highbd), the four
 * svt_av1_apply_(zz_based_)temporal_filter_planewise_medium(_hbd) functions, get_final_filtered_pixels, and the block walk
 * of produce_temporally_filtered_pic) on deterministic inputs (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C, compiled straight from its tree (REF = the reference checkout, run from the repository
 * root; the binary goes outside the repository).  EbTemporalFiltering.c is included below, not linked: its three tables
 * and apply_filtering_block_plane_wise are static there.
 *
 *   S=$REF/Source; C=$S/Lib/Common/Codec; E=$S/Lib/Encoder; INC="-I$S/API -I$C -I$S/Lib/Common/C_DEFAULT -I$E/Codec \
 *     -I$E/C_DEFAULT -I$E/Globals -I$S/Lib/Common/ASM_AVX2 -I$E/ASM_AVX2 -I$S/Lib/Common/ASM_SSE2 \
 *     -I$S/Lib/Common/ASM_SSE4_1 -I$REF/third_party/aom/inc -I$REF/third_party/cpuinfo/include -I$REF"
 *   gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -c $E/ASM_AVX2/EbTemporalFiltering_AVX2.c \
 *     -o /tmp/tf_avx2.o
 *   gcc -O2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -Ioracle/ref_harness \
 *     tests/golden/gen_golden_tf.c /tmp/tf_avx2.o $E/Codec/aom_dsp_rtcd.c $C/common_dsp_rtcd.c $C/EbUtility.c \
 *     $E/Codec/noise_util.c -o /tmp/gen_golden_tf -Wl,--gc-sections -lm -lpthread
 *   /tmp/gen_golden_tf tests/golden/tf.bin
 *   /tmp/gen_golden_tf --time        # scripts/tf_perf.py's workloads through the reference's C (and AVX2), one core
 *
 * (noise_util.c holds OD_DIVU's table, tf_avx2.o the reference's AVX2 functions, which are only compared.)
 *
 * Inputs that tests/tf_cases.py rebuilds instead of reading are "drawn": sample i of stream `seed` is
 * SplitMix64(seed + (i + 1) * 0x9E3779B97F4A7C15) % mod, golden_io.h's generator started at seed + i * the constant.
 *
 * Records (golden_io format):
 *   tab_log1p i32[225], tab_sqrt u32[16], tab_expf i32[113]   the three tables as compiled
 *   log1p     i32[n][2]    {noise_level_fp16, svt_aom_noise_log1p_fp16 of it}: both sides of base <= 0 and of 7.0, a sweep
 *                          (no base in 1..2047: the interpolation from log1p_tab_fp16[0] = INT32_MIN overflows an int there)
 *   decay     i64[n][4]    {decay_control, noise_log1p_fp16, q, tf_decay_factor_fp16}: the arithmetic of
 *                          produce_temporally_filtered_pic (:2913-2927), which is inline there, restated by this file
 *   divu      i32[1]       1: OD_DIVU_SMALL(x, 1000) == x / 1000 for every x <= 1000 * 65535 + 500 (checked here)
 *   nnoise, n<i>_par i32[5] {bd, w, h, content, seed}, n<i>_src (absent for the drawn 640x360 planes), n<i>_out i32[1]
 *             content 0 smooth + noise (drawn), 1 all edge (-65536), 2 / 3 all edge but 15 / 16 smooth samples, 4 constant
 *   nblock, b<i>_par i32[11] {bd, block_width, zz, tf_chroma, idx_32x32, mv_dist_th, content, prefill, seed, meta, decayset}
 *             b<i>_decay u32[3], _split i32[4], _mv32 i16[4][2] (x, y), _mv16 i16[16][2], _err32 u64[4], _err16 u64[16],
 *             _accum<p> u32[bh][bw], _count<p> u16[bh][bw] after the call.  src / pre are drawn (content 0: pre = src +- 16
 *             (x 4 at 10 bits), 1: independent, 2: src 0 / pre max, 3: src max / pre 0); prefill 1: accum = 1000 * src,
 *             count = 1000 before the call, else 0.  meta 0: the MeContext of TemporalFilterTestPlanewise.cc:55-125
 *             (errors x 16 at 10 bits), 1: zero motion, small errors, 2: motion (2000, -2000) / (1500, 900).
 *   b<i>_wide i32[1]       1: the record's 32-bit avg_err product (combined >> 3) * (d_factor >> 3) passes 2^32 in some
 *                          quadrant.  Legal inputs reach that (no FP_ASSERT of the reference fires): the extreme contents
 *                          with meta 2 and mv_dist_th 16 do, and the generator stops unless one record does.
 *   ncentral, c<i>_par i32[3] {bd, tf_chroma, seed}, c<i>_accum<p>, c<i>_count<p>   64x64 blocks, src drawn, stride 80
 *   nfinal, e<i>_par i32[3] {bd, mode, seed}, e<i>_out<p> [64][64] / [32][32]   mode 0: count 1000, accum 1000 * v (OD_DIVU's
 *             table branch); 1: count = 1000 + drawn % 26001, accum = v * count + drawn % count
 *   nframe, f<i>_par i32[8] {bd, w, h, n_refs, zz, tf_chroma, mv_dist_th, seed}, f<i>_decay u32[3],
 *             f<i>_split i32[n_refs][nblk][4], _mv32 i16[..][4][2], _mv16 i16[..][16][2], _err32 u64[..][4], _err16 u64[..][16],
 *             f<i>_out<p> [h][w]   centre and predictors drawn over 192x128; the walk is produce_temporally_filtered_pic's
 *             (:2939-3301): centre, per reference the four apply_filtering_block_plane_wise calls, final; in place.
 *
 * Where the CPU has AVX2 every record is made a second time through the reference's _avx2 functions and must be equal,
 * or the generator stops.  One exception: the AVX2 planewise functions have a 32- and a 16-wide path only, so the 8-wide
 * chroma planes of a block_width 16 record are the _c functions' alone (luma is still compared).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbTemporalFiltering.c"
#include "common_dsp_rtcd.h"
#include "golden_io.h"

static int g_avx2; /* the pass: 0 the _c functions, 1 the _avx2 ones */

static void bind_kernels(int avx2) {
    g_avx2    = avx2;
    svt_log2f = svt_aom_log2f_32;
    svt_av1_apply_temporal_filter_planewise_medium = avx2 ? svt_av1_apply_temporal_filter_planewise_medium_avx2
                                                          : svt_av1_apply_temporal_filter_planewise_medium_c;
    svt_av1_apply_temporal_filter_planewise_medium_hbd = avx2 ? svt_av1_apply_temporal_filter_planewise_medium_hbd_avx2
                                                              : svt_av1_apply_temporal_filter_planewise_medium_hbd_c;
    svt_av1_apply_zz_based_temporal_filter_planewise_medium =
        avx2 ? svt_av1_apply_zz_based_temporal_filter_planewise_medium_avx2
             : svt_av1_apply_zz_based_temporal_filter_planewise_medium_c;
    svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd =
        avx2 ? svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_avx2
             : svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_c;
    get_final_filtered_pixels      = avx2 ? svt_aom_get_final_filtered_pixels_avx2 : svt_aom_get_final_filtered_pixels_c;
    apply_filtering_central        = avx2 ? svt_aom_apply_filtering_central_avx2 : svt_aom_apply_filtering_central_c;
    apply_filtering_central_highbd = avx2 ? svt_aom_apply_filtering_central_highbd_avx2
                                          : svt_aom_apply_filtering_central_highbd_c;
    svt_estimate_noise_fp16        = avx2 ? svt_estimate_noise_fp16_avx2 : svt_estimate_noise_fp16_c;
    svt_estimate_noise_highbd_fp16 = avx2 ? svt_estimate_noise_highbd_fp16_avx2 : svt_estimate_noise_highbd_fp16_c;
}

static uint32_t draw(uint64_t seed, uint64_t i, uint32_t mod) {
    Rng r = {seed + i * 0x9E3779B97F4A7C15ull};
    return (uint32_t)(rng_next(&r) % mod);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* the output side: the first pass writes a record, the AVX2 pass compares with what the first pass kept */
typedef struct Keep {
    void  *data;
    size_t bytes;
} Keep;
static Keep       *g_keep;
static int         g_nkeep, g_ikeep, g_c_only; /* g_c_only: the next records have no AVX2 counterpart */
static GoldenFile *g_file;
static void        out_put(const char *name, char dt, int ndim, const uint32_t *dims, const void *data) {
    size_t n = golden_dsize(dt);
    for (int i = 0; i < ndim; i++) n *= dims[i];
    if (!g_avx2) {
        golden_put(g_file, name, dt, ndim, dims, data);
        g_keep                = realloc(g_keep, sizeof(Keep) * (g_nkeep + 1));
        g_keep[g_nkeep].data  = malloc(n ? n : 1);
        g_keep[g_nkeep].bytes = n;
        memcpy(g_keep[g_nkeep++].data, data, n);
    } else {
        if (g_ikeep >= g_nkeep || g_keep[g_ikeep].bytes != n || (!g_c_only && memcmp(g_keep[g_ikeep].data, data, n)))
            fprintf(stderr, "avx2 != c: record %s\n", name), exit(3);
        g_ikeep++;
    }
}
static void out1(const char *name, char dt, uint32_t n0, const void *d) { out_put(name, dt, 1, &n0, d); }
static void out2(const char *name, char dt, uint32_t n0, uint32_t n1, const void *d) {
    uint32_t dims[2] = {n0, n1};
    out_put(name, dt, 2, dims, d);
}
static void out3(const char *name, char dt, uint32_t n0, uint32_t n1, uint32_t n2, const void *d) {
    uint32_t dims[3] = {n0, n1, n2};
    out_put(name, dt, 3, dims, d);
}
static void out4(const char *name, char dt, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, const void *d) {
    uint32_t dims[4] = {n0, n1, n2, n3};
    out_put(name, dt, 4, dims, d);
}
static const char *nm(const char *fmt, int i, int p) {
    static char b[4][48];
    static int  k;
    k = (k + 1) & 3;
    snprintf(b[k], sizeof b[k], fmt, i, p);
    return b[k];
}
/* a cropped plane of 16-bit working samples as u8 / u16 */
static void out_plane(const char *name, int bd, int h, int w, const uint16_t *a, int stride) {
    if (bd > 8) {
        uint16_t *t = malloc(sizeof(uint16_t) * w * h);
        for (int y = 0; y < h; y++) memcpy(t + y * w, a + y * stride, sizeof(uint16_t) * w);
        out2(name, 'H', h, w, t);
        free(t);
    } else {
        uint8_t *t = malloc((size_t)w * h);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) t[y * w + x] = (uint8_t)a[y * stride + x];
        out2(name, 'B', h, w, t);
        free(t);
    }
}

/* ---- tables, log1p, decay, OD_DIVU ---- */
static void gen_tables(void) {
    out1("tab_log1p", 'i', sizeof(log1p_tab_fp16) / sizeof(log1p_tab_fp16[0]), log1p_tab_fp16);
    out1("tab_sqrt", 'I', 16, sqrt_array_fp16);
    out1("tab_expf", 'i', sizeof(expf_tab_fp16) / sizeof(expf_tab_fp16[0]), expf_tab_fp16);
    int32_t rows[160][2];
    int     n = 0;
    static const int32_t edge[] = {-2147483647 - 1, -1000000, -65537, -65536, -63488, -63487, -1, 0, 1, 2047, 2048, 65536,
                                   393215, 393216, 393217, 400000, 1000000, 20000000};
    for (size_t i = 0; i < sizeof edge / sizeof edge[0]; i++) rows[n++][0] = edge[i];
    for (int i = 0; i < 128; i++) rows[n++][0] = -63000 + i * 3803 + (int)draw(0x5446000000000001ull, i, 2048);
    for (int i = 0; i < n; i++)
        rows[i][1] = rows[i][0] == -2147483647 - 1 ? -2147483647 - 1 : svt_aom_noise_log1p_fp16(rows[i][0]);
    out2("log1p", 'i', n, 2, rows);

    int64_t   dec[64][4];
    int       m       = 0;
    const int qs[]    = {0, 1, 60, 127, 128, 129, 200, 255};
    const int ctl[]   = {1, 3, 4, 6};
    const int noise[] = {-70000, 0, 30000, 72000, 127527};
    for (size_t a = 0; a < 8; a++)
        for (size_t b = 0; b < 4; b++) {
            const int     q = qs[a], dc = ctl[b], nl = noise[(a + b) % 5];
            uint32_t      q_decay_fp8  = q >= TF_QINDEX_CUTOFF ? (uint32_t)(q * q) >> 5 : (uint32_t)MAX(q << 2, 1);
            const int32_t n_decay_fp10 = (dc * (45875 + nl)) / ((int32_t)1 << 6);
            dec[m][0] = dc, dec[m][1] = nl, dec[m][2] = q;
            dec[m++][3] = (uint32_t)(((((int64_t)n_decay_fp10) * ((int64_t)n_decay_fp10)) * q_decay_fp8) >> 11);
        }
    out2("decay", 'q', m, 4, dec);

    int32_t ok = 1;
    for (uint32_t x = 0; x <= 1000u * 65535u + 500u; x++)
        if (OD_DIVU_SMALL(x, 1000) != x / 1000) ok = 0;
    if (!ok) fprintf(stderr, "OD_DIVU_SMALL(x, 1000) differs from x / 1000\n"), exit(3);
    out1("divu", 'i', 1, &ok);
}

/* ---- noise ---- */
static void fill_noise(uint16_t *a, int bd, int w, int h, int content, uint64_t seed) {
    const int maxv = (1 << bd) - 1, sc = 1 << (bd - 8);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int v;
            switch (content) {
            case 0: v = clampi((x + 2 * y) * sc / 8 + (int)draw(seed, (uint64_t)y * w + x, 10 * sc), 0, maxv); break;
            case 4: v = 77 * sc; break;
            default: v = x & 2 ? maxv : 0; break;
            }
            a[y * w + x] = (uint16_t)v;
        }
    if (content == 2 || content == 3) { /* a flat patch of three rows: its middle row's interior is smooth */
        const int n = content == 2 ? 15 : 16;
        for (int y = 10; y < 13; y++)
            for (int x = 8; x < 8 + n + 2; x++) a[y * w + x] = (uint16_t)(maxv / 2);
    }
}
static int32_t run_noise(const uint16_t *a, int bd, int w, int h) {
    if (bd > 8) return svt_estimate_noise_highbd_fp16(a, w, h, w, bd);
    uint8_t *b = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++) b[i] = (uint8_t)a[i];
    const int32_t r = svt_estimate_noise_fp16(b, (uint16_t)w, (uint16_t)h, (uint16_t)w);
    free(b);
    return r;
}
static void gen_noise(void) {
    static const int sizes[3][2] = {{64, 48}, {67, 35}, {640, 360}};
    int              n           = 0;
    for (int bd = 8; bd <= 10; bd += 2)
        for (int s = 0; s < 3; s++)
            for (int content = 0; content < 5; content++) {
                if (s == 2 && content) continue;
                const int      w = sizes[s][0], h = sizes[s][1];
                const uint64_t seed = 0x5446000000000100ull + n;
                uint16_t      *a    = malloc(sizeof(uint16_t) * w * h);
                fill_noise(a, bd, w, h, content, seed);
                int32_t r = run_noise(a, bd, w, h), par[5] = {bd, w, h, content, n};
                if ((content == 1 || content == 2) && r != -65536) fprintf(stderr, "noise %d: smooth samples\n", n), exit(3);
                if ((content == 3 || content == 4) && r != 0) fprintf(stderr, "noise %d: not flat\n", n), exit(3);
                if (content == 0 && r <= 0) fprintf(stderr, "noise %d: no estimate\n", n), exit(3);
                out1(nm("n%d_par", n, 0), 'i', 5, par);
                if (s != 2) out_plane(nm("n%d_src", n, 0), bd, h, w, a, w);
                out1(nm("n%d_out", n, 0), 'i', 1, &r);
                free(a);
                n++;
            }
    int32_t nn = n;
    out1("nnoise", 'i', 1, &nn);
}

/* ---- the RTCD-granularity records ---- */
typedef struct Meta {
    int32_t  split[4];
    int16_t  mv32[4][2], mv16[16][2];
    uint64_t err32[4], err16[16];
} Meta;
static void meta_to_ctx(const Meta *m, MeContext *c) {
    for (int i = 0; i < 4; i++) {
        c->tf_32x32_block_split_flag[i] = m->split[i];
        c->tf_32x32_mv_x[i] = m->mv32[i][0], c->tf_32x32_mv_y[i] = m->mv32[i][1];
        c->tf_32x32_block_error[i] = m->err32[i];
    }
    for (int i = 0; i < 16; i++) {
        c->tf_16x16_mv_x[i] = m->mv16[i][0], c->tf_16x16_mv_y[i] = m->mv16[i][1];
        c->tf_16x16_block_error[i] = m->err16[i];
    }
}
static void meta_set(Meta *m, int kind, int bd) {
    static const int e16[16] = {29087, 28482, 44508, 42356, 35319, 37670, 38551, 39320,
                                28360, 32753, 38335, 50679, 44700, 49620, 47070, 41171};
    static const int e32[4]  = {156756, 168763, 143351, 189005};
    static const int x16[16] = {160, 13, 13, 13, 44, 12, 1, 13, 12, 52, 11, 52, -20, 13, 11, -4};
    static const int y16[16] = {-390, -35, -38, -60, -33, -19, -35, -34, -39, -19, -39, 21, -52, -31, -12, -36};
    static const int x32[4] = {-196, -188, -228, -220}, y32[4] = {-436, -436, -436, -420};
    const int        sh = bd > 8 ? 4 : 0;
    for (int i = 0; i < 4; i++) {
        m->split[i]   = !(i & 1);
        m->err32[i]   = (uint64_t)(kind == 1 ? 900 + 77 * i : e32[i]) << sh;
        m->mv32[i][0] = (int16_t)(kind == 0 ? x32[i] : kind == 1 ? 0 : 1500);
        m->mv32[i][1] = (int16_t)(kind == 0 ? y32[i] : kind == 1 ? 0 : 900);
    }
    for (int i = 0; i < 16; i++) {
        m->err16[i]   = (uint64_t)(kind == 1 ? 300 + 31 * i : e16[i]) << sh;
        m->mv16[i][0] = (int16_t)(kind == 0 ? x16[i] : kind == 1 ? (i == 5 ? 3 : 0) : 2000);
        m->mv16[i][1] = (int16_t)(kind == 0 ? y16[i] : kind == 1 ? (i == 6 ? -1 : 0) : -2000);
    }
}
static void decay_set(uint32_t d[3], int set) {
    static const uint32_t v[3][3] = {{6000000, 9000000, 12000000}, {500, 1023, 1024}, {150000, 200000, 250000}};
    memcpy(d, v[set], sizeof v[set]);
}

/* does a quadrant's (combined >> 3) * (d_factor >> 3) pass 2^32?  Found from the outside: the weight the reference gave
 * (count's increment) against the one a 64-bit product gives, recomputed with the reference's own pieces */
static int product_is_wide(const MeContext *c, int idx, const uint16_t *src, const uint16_t *pre, int stride, int bw, int bd) {
    const uint32_t thr = AOMMAX((c->tf_mv_dist_th << 16) / 10, 1 << 16);
    int            wide = 0;
    for (int q = 0; q < 4; q++) {
        const int split = c->tf_32x32_block_split_flag[idx];
        const int col = split ? c->tf_16x16_mv_x[idx * 4 + q] : c->tf_32x32_mv_x[idx];
        const int row = split ? c->tf_16x16_mv_y[idx * 4 + q] : c->tf_32x32_mv_y[idx];
        const uint32_t d = AOMMAX((sqrt_fast(((uint32_t)(col * col + row * row)) << 8) << 12) / (thr >> 8), 1 << 8);
        uint32_t       sum = 0;
        const int      hw = bw / 2, x0 = (q & 1) * hw, y0 = (q >> 1) * hw;
        for (int y = 0; y < hw; y++)
            for (int x = 0; x < hw; x++) {
                const int df = src[(y0 + y) * stride + x0 + x] - pre[(y0 + y) * stride + x0 + x];
                sum += (uint32_t)(df * df);
            }
        sum >>= 2 * (bd - 8);
        const uint32_t we = (((sum << 4) / hw) << 4) / hw;
        const uint32_t be = split ? (uint32_t)(c->tf_16x16_block_error[idx * 4 + q] >> (bd > 8 ? 4 : 0))
                                  : (uint32_t)(c->tf_32x32_block_error[idx] >> (bd > 8 ? 6 : 2));
        const uint64_t comb = (we * 5 + be) / 6;
        wide |= (comb >> 3) * (uint64_t)(d >> 3) >= ((uint64_t)1 << 32);
    }
    return wide;
}

#define BS 64 /* stride of every buffer of a block record */
static int gen_blocks(void) {
    /* {block_width, zz, tf_chroma, idx_32x32, mv_dist_th, content, prefill, meta, decayset} */
    static const int cases[][9] = {
        {32, 0, 1, 0, 1080, 0, 0, 0, 0}, {32, 0, 1, 1, 1080, 0, 1, 0, 0}, {32, 0, 1, 2, 1080, 1, 0, 0, 2},
        {32, 0, 1, 3, 1080, 2, 0, 0, 0}, {32, 0, 1, 1, 16, 3, 0, 2, 0},   {32, 0, 1, 0, 16, 0, 1, 2, 0},
        {32, 0, 1, 2, 16, 2, 0, 2, 2},   {32, 0, 0, 0, 1080, 0, 0, 1, 0}, {32, 0, 1, 1, 1080, 0, 0, 1, 1},
        {32, 0, 1, 2, 1080, 0, 1, 1, 2}, {16, 0, 1, 0, 1080, 0, 0, 0, 0}, {16, 0, 1, 1, 16, 1, 1, 2, 2},
        {16, 0, 0, 3, 1080, 0, 0, 1, 0}, {32, 1, 1, 0, 1080, 0, 0, 0, 0}, {32, 1, 1, 1, 1080, 0, 1, 0, 2},
        {32, 1, 0, 2, 1080, 1, 0, 1, 1}, {16, 1, 1, 3, 1080, 0, 0, 0, 0}, {16, 1, 1, 0, 1080, 0, 1, 1, 2}};
    const int  ncase = (int)(sizeof cases / sizeof cases[0]);
    int        n = 0, any_wide = 0;
    MeContext *ctx = calloc(1, sizeof *ctx);
    for (int bd = 8; bd <= 10; bd += 2)
        for (int k = 0; k < ncase; k++, n++) {
            const int *c = cases[k], bw = c[0], zz = c[1], chroma = c[2], idx = c[3], content = c[5], prefill = c[6];
            const int  maxv = (1 << bd) - 1, sc = 1 << (bd - 8);
            const uint64_t seed = 0x5446000000001000ull + 16 * (uint64_t)n;
            uint16_t       src[3][BS * BS], pre[3][BS * BS], cnt[3][BS * BS];
            uint32_t       acc[3][BS * BS];
            uint8_t        s8[3][BS * BS], p8[3][BS * BS];
            Meta           m;
            meta_set(&m, c[7], bd);
            meta_to_ctx(&m, ctx);
            decay_set(ctx->tf_decay_factor_fp16, c[8]);
            ctx->tf_block_col = idx & 1, ctx->tf_block_row = idx >> 1;
            ctx->tf_mv_dist_th = (uint16_t)c[4], ctx->tf_chroma = (uint8_t)chroma;
            memset(acc, 0, sizeof acc), memset(cnt, 0, sizeof cnt);
            for (int p = 0; p < 3; p++) {
                const int w = p ? bw / 2 : bw;
                for (int y = 0; y < w; y++)
                    for (int x = 0; x < w; x++) {
                        const int i = y * w + x, o = y * BS + x;
                        int       s = (int)draw(seed + p, i, maxv + 1), q;
                        switch (content) {
                        case 0: q = clampi(s - 16 * sc + (int)draw(seed + 4 + p, i, 32 * sc), 0, maxv); break;
                        case 1: q = (int)draw(seed + 4 + p, i, maxv + 1); break;
                        case 2: s = 0, q = maxv; break;
                        default: s = maxv, q = 0; break;
                        }
                        src[p][o] = (uint16_t)s, pre[p][o] = (uint16_t)q, s8[p][o] = (uint8_t)s, p8[p][o] = (uint8_t)q;
                        if (prefill && (p == 0 || chroma)) acc[p][o] = 1000u * s, cnt[p][o] = 1000;
                    }
            }
            if (bd == 8 && zz)
                svt_av1_apply_zz_based_temporal_filter_planewise_medium(ctx, p8[0], BS, p8[1], p8[2], BS, bw, bw, 1, 1, acc[0],
                                                                        cnt[0], acc[1], cnt[1], acc[2], cnt[2]);
            else if (bd == 8)
                svt_av1_apply_temporal_filter_planewise_medium(ctx, s8[0], BS, p8[0], BS, s8[1], s8[2], BS, p8[1], p8[2], BS,
                                                               bw, bw, 1, 1, acc[0], cnt[0], acc[1], cnt[1], acc[2], cnt[2]);
            else if (zz)
                svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd(ctx, pre[0], BS, pre[1], pre[2], BS, bw, bw, 1, 1,
                                                                            acc[0], cnt[0], acc[1], cnt[1], acc[2], cnt[2], bd);
            else
                svt_av1_apply_temporal_filter_planewise_medium_hbd(ctx, src[0], BS, pre[0], BS, src[1], src[2], BS, pre[1],
                                                                   pre[2], BS, bw, bw, 1, 1, acc[0], cnt[0], acc[1], cnt[1],
                                                                   acc[2], cnt[2], bd);
            int32_t par[11] = {bd, bw, zz, chroma, idx, c[4], content, prefill, n, c[7], c[8]};
            int32_t wide    = !zz && product_is_wide(ctx, idx, src[0], pre[0], BS, bw, bd);
            any_wide |= wide;
            out1(nm("b%d_par", n, 0), 'i', 11, par);
            out1(nm("b%d_wide", n, 0), 'i', 1, &wide);
            out1(nm("b%d_decay", n, 0), 'I', 3, ctx->tf_decay_factor_fp16);
            out1(nm("b%d_split", n, 0), 'i', 4, m.split);
            out2(nm("b%d_mv32", n, 0), 'h', 4, 2, m.mv32);
            out2(nm("b%d_mv16", n, 0), 'h', 16, 2, m.mv16);
            out1(nm("b%d_err32", n, 0), 'Q', 4, m.err32);
            out1(nm("b%d_err16", n, 0), 'Q', 16, m.err16);
            for (int p = 0; p < 3; p++) {
                const int w = p ? bw / 2 : bw;
                uint32_t  a[32 * 32];
                uint16_t  t[32 * 32];
                for (int y = 0; y < w; y++)
                    for (int x = 0; x < w; x++) a[y * w + x] = acc[p][y * BS + x], t[y * w + x] = cnt[p][y * BS + x];
                g_c_only = p && bw == 16 && chroma;
                out2(nm("b%d_accum%d", n, p), 'I', w, w, a);
                out2(nm("b%d_count%d", n, p), 'H', w, w, t);
                g_c_only = 0;
            }
        }
    if (!any_wide) fprintf(stderr, "no block record's avg_err product passes 2^32\n"), exit(3);
    int32_t nn = n;
    out1("nblock", 'i', 1, &nn);
    free(ctx);
    return n;
}

#define CS 80 /* luma stride of the central / final records */
static void gen_central_final(void) {
    MeContext          *ctx = calloc(1, sizeof *ctx);
    EbPictureBufferDesc desc;
    memset(&desc, 0, sizeof desc);
    desc.stride_y = CS;
    static const int cc[3][2] = {{8, 1}, {10, 1}, {10, 0}};
    for (int i = 0; i < 3; i++) {
        const int      bd = cc[i][0], chroma = cc[i][1], maxv = (1 << bd) - 1;
        const uint64_t seed = 0x5446000000002000ull + 16 * (uint64_t)i;
        uint16_t       s16[3][64 * CS], cnt[3][BLK_PELS];
        uint8_t        s8[3][64 * CS];
        uint32_t       acc[3][BLK_PELS];
        memset(acc, 0, sizeof acc), memset(cnt, 0, sizeof cnt);
        for (int p = 0; p < 3; p++) {
            const int w = p ? 32 : 64, st = p ? CS / 2 : CS;
            for (int y = 0; y < w; y++)
                for (int x = 0; x < w; x++) {
                    const int v        = (int)draw(seed + p, y * w + x, maxv + 1);
                    s16[p][y * st + x] = (uint16_t)v, s8[p][y * st + x] = (uint8_t)v;
                }
        }
        uint32_t *a[3] = {acc[0], acc[1], acc[2]};
        uint16_t *c[3] = {cnt[0], cnt[1], cnt[2]}, *s16p[3] = {s16[0], s16[1], s16[2]};
        uint8_t  *s8p[3] = {s8[0], s8[1], s8[2]};
        ctx->tf_chroma   = (uint8_t)chroma;
        if (bd == 8)
            apply_filtering_central(ctx, &desc, s8p, a, c, 64, 64, 1, 1);
        else
            apply_filtering_central_highbd(ctx, &desc, s16p, a, c, 64, 64, 1, 1);
        int32_t par[3] = {bd, chroma, i};
        out1(nm("c%d_par", i, 0), 'i', 3, par);
        for (int p = 0; p < 3; p++) {
            const int w = p ? 32 : 64;
            out2(nm("c%d_accum%d", i, p), 'I', w, w, acc[p]);
            out2(nm("c%d_count%d", i, p), 'H', w, w, cnt[p]);
        }
    }
    int32_t nc = 3;
    out1("ncentral", 'i', 1, &nc);

    static const int fc[4][2] = {{8, 0}, {8, 1}, {10, 0}, {10, 1}};
    for (int i = 0; i < 4; i++) {
        const int      bd = fc[i][0], mode = fc[i][1], maxv = (1 << bd) - 1;
        const uint64_t seed = 0x5446000000003000ull + 16 * (uint64_t)i;
        uint16_t       o16[3][72 * CS], cnt[3][BLK_PELS];
        uint8_t        o8[3][72 * CS];
        uint32_t       acc[3][BLK_PELS];
        memset(o16, 0, sizeof o16), memset(o8, 0, sizeof o8);
        for (int p = 0; p < 3; p++) {
            const int w = p ? 32 : 64;
            for (int k = 0; k < w * w; k++) {
                const uint32_t v = draw(seed + p, k, maxv); /* < maxv: the rounded quotient stays in range */
                const uint32_t c = mode ? 1000 + draw(seed + 4 + p, k, 26001) : 1000;
                cnt[p][k] = (uint16_t)c, acc[p][k] = mode ? v * c + draw(seed + 8 + p, k, c) : v * c;
            }
        }
        uint32_t      *a[3] = {acc[0], acc[1], acc[2]};
        uint16_t      *c[3] = {cnt[0], cnt[1], cnt[2]}, *o16p[3] = {o16[0], o16[1], o16[2]};
        uint8_t       *o8p[3] = {o8[0], o8[1], o8[2]};
        const uint32_t stride[3] = {CS, CS / 2, CS / 2};
        ctx->tf_chroma = 1;
        /* the block at (8, 4) luma, (4, 2) chroma of the picture */
        get_final_filtered_pixels(ctx, o8p, o16p, a, c, stride, 4 * CS + 8, 2 * (CS / 2) + 4, 32, 32, bd > 8);
        int32_t par[3] = {bd, mode, i};
        out1(nm("e%d_par", i, 0), 'i', 3, par);
        for (int p = 0; p < 3; p++) {
            const int w = p ? 32 : 64, st = p ? CS / 2 : CS, off = p ? 2 * st + 4 : 4 * st + 8;
            uint16_t  t[64 * CS];
            for (int k = 0; k < w * st; k++) t[k] = bd > 8 ? o16[p][off + k] : o8[p][off + k];
            out_plane(nm("e%d_out%d", i, p), bd, w, w, t, st);
        }
    }
    int32_t nf = 4;
    out1("nfinal", 'i', 1, &nf);
    free(ctx);
}

/* ---- whole pictures: produce_temporally_filtered_pic's block walk (:2939-3301) with the motion half replaced by
 * given predictor pictures and metadata ---- */
typedef struct Pic {
    uint16_t *p16[3];
    uint8_t  *p8[3];
    int       stride[3], aw, ah; /* the 64-aligned area */
} Pic;
static void pic_alloc(Pic *p, int w, int h) {
    p->aw = (w + 63) & ~63, p->ah = (h + 63) & ~63;
    for (int k = 0; k < 3; k++) {
        p->stride[k] = p->aw >> (k > 0);
        const size_t n = (size_t)p->stride[k] * (p->ah >> (k > 0));
        p->p16[k] = malloc(sizeof(uint16_t) * n), p->p8[k] = malloc(n);
    }
}
static void pic_free(Pic *p) {
    for (int k = 0; k < 3; k++) free(p->p16[k]), free(p->p8[k]);
}
static void pic_set(Pic *p, int k, size_t i, int v) { p->p16[k][i] = (uint16_t)v, p->p8[k][i] = (uint8_t)v; }

static void filter_picture(MeContext *ctx, int bd, int w, int h, Pic *centre, Pic *refs, int n_refs, const Meta *meta) {
    DECLARE_ALIGNED(32, uint32_t, accumulator[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, counter[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint16_t, pr16[BLK_PELS * COLOR_CHANNELS]);
    DECLARE_ALIGNED(32, uint8_t, pr8[BLK_PELS * COLOR_CHANNELS]);
    uint32_t *accum[3] = {accumulator, accumulator + BLK_PELS, accumulator + 2 * BLK_PELS};
    uint16_t *count[3] = {counter, counter + BLK_PELS, counter + 2 * BLK_PELS};
    uint16_t *pred16[3] = {pr16, pr16 + BLK_PELS, pr16 + 2 * BLK_PELS};
    uint8_t  *pred8[3] = {pr8, pr8 + BLK_PELS, pr8 + 2 * BLK_PELS};
    uint32_t  stride[3] = {centre->stride[0], centre->stride[1], centre->stride[2]}, stride_pred[3] = {BW, BW / 2, BW / 2};
    EbPictureBufferDesc desc;
    memset(&desc, 0, sizeof desc);
    desc.stride_y      = (uint16_t)stride[0];
    const int blk_cols = (w + BW - 1) / BW, blk_rows = (h + BH - 1) / BH;
    for (int br = 0; br < blk_rows; br++)
        for (int bc = 0; bc < blk_cols; bc++) {
            const int yoff = bc * BW + br * BH * stride[0], coff = bc * (BW / 2) + br * (BH / 2) * stride[1];
            uint8_t  *s8[3] = {centre->p8[0] + yoff, centre->p8[1] + coff, centre->p8[2] + coff};
            uint16_t *s16[3] = {centre->p16[0] + yoff, centre->p16[1] + coff, centre->p16[2] + coff};
            memset(accumulator, 0, sizeof accumulator), memset(counter, 0, sizeof counter);
            if (bd == 8)
                apply_filtering_central(ctx, &desc, s8, accum, count, BW, BH, 1, 1);
            else
                apply_filtering_central_highbd(ctx, &desc, s16, accum, count, BW, BH, 1, 1);
            for (int r = 0; r < n_refs; r++) {
                for (int p = 0; p < 3; p++) { /* the predictor block the motion compensation would have left */
                    const int bwp = p ? BW / 2 : BW, off = p ? coff : yoff;
                    for (int y = 0; y < bwp; y++) {
                        memcpy(pred16[p] + y * bwp, refs[r].p16[p] + off + y * stride[p], sizeof(uint16_t) * bwp);
                        memcpy(pred8[p] + y * bwp, refs[r].p8[p] + off + y * stride[p], bwp);
                    }
                }
                meta_to_ctx(&meta[r * blk_cols * blk_rows + br * blk_cols + bc], ctx);
                for (int row = 0; row < 2; row++)
                    for (int col = 0; col < 2; col++) {
                        ctx->tf_block_col = col, ctx->tf_block_row = row;
                        apply_filtering_block_plane_wise(ctx, row, col, s8, s16, pred8, pred16, accum, count, stride,
                                                         stride_pred, BW >> 1, BH >> 1, 1, 1, bd);
                    }
            }
            get_final_filtered_pixels(ctx, centre->p8, centre->p16, accum, count, stride, yoff, coff, BW / 2, BH / 2, bd > 8);
        }
}

/* drawn centre and predictor pictures over the aligned area */
static void draw_pictures(int bd, uint64_t seed, Pic *centre, Pic *refs, int n_refs) {
    const int maxv = (1 << bd) - 1, sc = 1 << (bd - 8);
    for (int p = 0; p < 3; p++) {
        const int w = centre->stride[p], h = centre->ah >> (p > 0);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const int    v = clampi((2 * x + y) * sc / 4 + (int)draw(seed + p, i, 64 * sc), 0, maxv);
                pic_set(centre, p, i, v);
                for (int r = 0; r < n_refs; r++) {
                    const int amp = (2 + 3 * r) * sc;
                    pic_set(&refs[r], p, i, clampi(v - amp + (int)draw(seed + 4 + 4 * r + p, i, 2 * amp + 1), 0, maxv));
                }
            }
    }
}
static void draw_meta(Meta *m, int n, int bd, Rng *r) {
    const int sh = bd > 8 ? 4 : 0;
    for (int k = 0; k < n; k++, m++) {
        for (int i = 0; i < 4; i++) {
            m->split[i] = (int32_t)rng_below(r, 2);
            const int z = !rng_below(r, 4);
            m->mv32[i][0] = (int16_t)(z ? 0 : (int)rng_below(r, 65) - 32), m->mv32[i][1] = (int16_t)(z ? 0 : (int)rng_below(r, 65) - 32);
            m->err32[i] = (uint64_t)rng_below(r, 200000) << sh;
        }
        for (int i = 0; i < 16; i++) {
            const int z = !rng_below(r, 4);
            m->mv16[i][0] = (int16_t)(z ? 0 : (int)rng_below(r, 65) - 32), m->mv16[i][1] = (int16_t)(z ? 0 : (int)rng_below(r, 65) - 32);
            m->err16[i] = (uint64_t)rng_below(r, 60000) << sh;
        }
    }
}

static void gen_frames(void) {
    /* {bd, n_refs, zz, tf_chroma, mv_dist_th} */
    static const int cases[][5] = {{8, 0, 0, 1, 1080}, {8, 1, 0, 1, 1080}, {8, 5, 0, 1, 12},  {8, 5, 0, 0, 1080},
                                   {10, 0, 0, 1, 1080}, {10, 1, 0, 1, 12},  {10, 5, 0, 1, 1080}, {10, 5, 1, 1, 1080}};
    const int        n = (int)(sizeof cases / sizeof cases[0]), w = 136, h = 72, nblk = 6;
    MeContext       *ctx = calloc(1, sizeof *ctx);
    Rng              r   = {0x5446000000004000ull};
    for (int i = 0; i < n; i++) {
        const int      bd = cases[i][0], nr = cases[i][1], zz = cases[i][2], chroma = cases[i][3];
        const uint64_t seed = 0x5446000000005000ull + 256 * (uint64_t)i;
        Pic            centre, refs[5];
        Meta          *meta = calloc((size_t)(nr ? nr : 1) * nblk, sizeof(Meta));
        pic_alloc(&centre, w, h);
        for (int k = 0; k < nr; k++) pic_alloc(&refs[k], w, h);
        draw_pictures(bd, seed, &centre, refs, nr);
        draw_meta(meta, nr * nblk, bd, &r);
        decay_set(ctx->tf_decay_factor_fp16, 0);
        ctx->tf_mv_dist_th = (uint16_t)cases[i][4], ctx->tf_chroma = (uint8_t)chroma;
        ctx->tf_ctrls.use_zz_based_filter = (uint8_t)zz;
        filter_picture(ctx, bd, w, h, &centre, refs, nr, meta);
        int32_t par[8] = {bd, w, h, nr, zz, chroma, cases[i][4], i};
        out1(nm("f%d_par", i, 0), 'i', 8, par);
        out1(nm("f%d_decay", i, 0), 'I', 3, ctx->tf_decay_factor_fp16);
        const int nm_ = nr * nblk;
        int32_t  *sp  = malloc(sizeof(int32_t) * 4 * (nm_ + 1));
        int16_t  *m32 = malloc(sizeof(int16_t) * 8 * (nm_ + 1)), *m16 = malloc(sizeof(int16_t) * 32 * (nm_ + 1));
        uint64_t *e32 = malloc(sizeof(uint64_t) * 4 * (nm_ + 1)), *e16 = malloc(sizeof(uint64_t) * 16 * (nm_ + 1));
        for (int k = 0; k < nm_; k++) {
            memcpy(sp + 4 * k, meta[k].split, 16), memcpy(m32 + 8 * k, meta[k].mv32, 16), memcpy(m16 + 32 * k, meta[k].mv16, 64);
            memcpy(e32 + 4 * k, meta[k].err32, 32), memcpy(e16 + 16 * k, meta[k].err16, 128);
        }
        out3(nm("f%d_split", i, 0), 'i', nr, nblk, 4, sp);
        out4(nm("f%d_mv32", i, 0), 'h', nr, nblk, 4, 2, m32);
        out4(nm("f%d_mv16", i, 0), 'h', nr, nblk, 16, 2, m16);
        out3(nm("f%d_err32", i, 0), 'Q', nr, nblk, 4, e32);
        out3(nm("f%d_err16", i, 0), 'Q', nr, nblk, 16, e16);
        free(sp), free(m32), free(m16), free(e32), free(e16);
        for (int p = 0; p < 3; p++) {
            if (bd == 8)
                for (size_t k = 0; k < (size_t)centre.stride[p] * (centre.ah >> (p > 0)); k++) centre.p16[p][k] = centre.p8[p][k];
            out_plane(nm("f%d_out%d", i, p), bd, h >> (p > 0), w >> (p > 0), centre.p16[p], centre.stride[p]);
        }
        pic_free(&centre);
        for (int k = 0; k < nr; k++) pic_free(&refs[k]);
        free(meta);
    }
    int32_t nn = n;
    out1("nframe", 'i', 1, &nn);
    free(ctx);
}

/* scripts/tf_perf.py's workloads through the reference's functions on one core */
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
static void time_reference(void) {
    static const int shapes[2][3] = {{8, 1920, 1080}, {10, 3840, 2160}};
    const int        nr = 6, passes = __builtin_cpu_supports("avx2") ? 2 : 1;
    for (int k = 0; k < 2; k++) {
        const int  bd = shapes[k][0], w = shapes[k][1], h = shapes[k][2];
        const int  nblk = ((w + 63) / 64) * ((h + 63) / 64);
        MeContext *ctx = calloc(1, sizeof *ctx);
        Pic        centre, refs[6];
        Meta      *meta = calloc((size_t)nr * nblk, sizeof(Meta));
        Rng        r = {0x5446000000006000ull};
        pic_alloc(&centre, w, h);
        for (int i = 0; i < nr; i++) pic_alloc(&refs[i], w, h);
        draw_meta(meta, nr * nblk, bd, &r);
        decay_set(ctx->tf_decay_factor_fp16, 0);
        ctx->tf_mv_dist_th = 1080, ctx->tf_chroma = 1;
        double ms[2] = {0, 0}, noise_ms[2] = {0, 0};
        for (int pass = 0; pass < passes; pass++) {
            bind_kernels(pass);
            double best = 1e30, nbest = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                draw_pictures(bd, 0x5446000000007000ull, &centre, refs, nr);
                double t0 = now_ms();
                filter_picture(ctx, bd, w, h, &centre, refs, nr, meta);
                double t1 = now_ms();
                volatile int32_t v = bd > 8 ? svt_estimate_noise_highbd_fp16(centre.p16[0], w, h, centre.stride[0], bd)
                                            : svt_estimate_noise_fp16(centre.p8[0], (uint16_t)w, (uint16_t)h, (uint16_t)centre.stride[0]);
                double t2 = now_ms();
                (void)v;
                if (t1 - t0 < best) best = t1 - t0;
                if (t2 - t1 < nbest) nbest = t2 - t1;
            }
            ms[pass] = best, noise_ms[pass] = nbest;
        }
        printf("{\"workload\": \"%dx%d %d-bit, %d references\", \"filter_c_ms\": %.2f, \"filter_avx2_ms\": %.2f, "
               "\"noise_c_ms\": %.2f, \"noise_avx2_ms\": %.2f, \"reps\": 3}\n", w, h, bd, nr, ms[0], ms[1], noise_ms[0], noise_ms[1]);
        pic_free(&centre);
        for (int i = 0; i < nr; i++) pic_free(&refs[i]);
        free(meta), free(ctx);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <out.bin> | --time\n", argv[0]);
        return 2;
    }
    if (!strcmp(argv[1], "--time")) {
        time_reference();
        return 0;
    }
    GoldenFile g = golden_open(argv[1]);
    g_file       = &g;
    const int passes = __builtin_cpu_supports("avx2") ? 2 : 1;
    int       nb     = 0;
    for (int pass = 0; pass < passes; pass++) {
        bind_kernels(pass);
        gen_tables();
        gen_noise();
        nb = gen_blocks();
        gen_central_final();
        gen_frames();
    }
    golden_close(&g);
    fprintf(stderr, "%d records, %d block records; %s\n", g_nkeep, nb,
            passes == 2 ? "every one equal through the AVX2 functions" : "no AVX2 on this host: the _c functions only");
    return 0;
}
