/*
 * gen_golden_resize.c — writes tests/golden/resize.bin: the reference's own non-normative frame resizer
 * (svt_av1_resize_plane_c, svt_av1_highbd_resize_plane_c, svt_aom_resize_frame; EbResize.c) on deterministic inputs
 * (test infrastructure; never shipped, not built by build()).
 *
 * It links the REFERENCE's C, compiled straight from its tree (REF = the reference checkout, run from the
 * repository root; the binary goes outside the repository).  EbResize.c is included below, not linked:
 * get_down2_steps, get_down2_length, choose_interp_filter and the _horizontal plane functions are static or
 * undeclared there.
 *
 *   S=$REF/Source; C=$S/Lib/Common/Codec; E=$S/Lib/Encoder; INC="-I$S/API -I$C -I$S/Lib/Common/C_DEFAULT -I$E/Codec \
 *     -I$E/C_DEFAULT -I$E/Globals -I$S/Lib/Common/ASM_AVX2 -I$E/ASM_AVX2 -I$S/Lib/Common/ASM_SSE2 \
 *     -I$S/Lib/Common/ASM_SSE4_1 -I$REF/third_party/aom/inc -I$REF/third_party/cpuinfo/include -I$REF"
 *   gcc -O2 -mavx2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -c $E/ASM_AVX2/resize_avx2.c \
 *     -o /tmp/resize_avx2.o
 *   gcc -O2 -ffunction-sections -fdata-sections -DARCH_X86_64=1 -w $INC -Ioracle/ref_harness \
 *     tests/golden/gen_golden_resize.c /tmp/resize_avx2.o $E/Codec/aom_dsp_rtcd.c $C/common_dsp_rtcd.c $C/EbUtility.c \
 *     $C/EbMalloc.c $C/EbLog.c $C/EbThreads.c $S/Lib/Common/C_DEFAULT/EbPictureOperators_C.c $C/EbSuperRes.c \
 *     $C/EbMcp.c -o /tmp/gen_golden_resize -Wl,--gc-sections -lm -lpthread
 *   /tmp/gen_golden_resize tests/golden/resize.bin
 *   /tmp/gen_golden_resize --time     # scripts/resize_perf.py's workloads through the reference's C, one core
 *
 * (EbSuperRes.c holds calculate_scaled_size_helper, EbMcp.c the padding svt_aom_resize_frame ends with, resize_avx2.o
 * the reference's AVX2 plane functions, which are only compared.)
 *
 * Records (golden_io format; tests/resize_cases.py reads them):
 *   filters           i16 [5][64][8]   svt_aom_av1_filteredinterp_filters500 / 625 / 750 / 875, av1_resize_filter_normative
 *   half_filters      i16 [2][4]       svt_aom_av1_down2_symeven_half_filter, av1_down2_symodd_half_filter
 *   plan              i32 [n][7]       {in_length, out_length, get_down2_steps, the length after those steps,
 *                                       the table choose_interp_filter picks for it (-1: no interpolation), delta, offset}
 *   scaled            i32 [9][4]       {denominator 9..17, calculate_scaled_size_helper of 88, 16, 44}
 *   nplane            i32 [1]
 *   p<i>_par          i32 [6]          {bit_depth, in_w, in_h, out_w, out_h, content (0 random, 1 extreme)}
 *   p<i>_src          u8 / u16 [in_h][in_w]
 *   p<i>_out          u8 / u16 [out_h][out_w]   svt_av1_resize_plane_c / svt_av1_highbd_resize_plane_c of it (the
 *                                       _horizontal function when out_h == in_h, as svt_aom_resize_frame picks it)
 *   clipped           i32 [nplane][2]  sums of the horizontal stage below 0 / above max before the clip (counted for the
 *                                       extreme records without a halving step; 0 elsewhere)
 *   nframe            i32 [1]
 *   f<i>_par          i32 [5]          {bit_depth, src_w, src_h, dst_w, dst_h}
 *   f<i>_src<p> / f<i>_out<p>          u8 / u16 planes (chroma (dim + 1) >> 1) before / after svt_aom_resize_frame
 *
 * Where the CPU has AVX2 the svt_av1_resize_plane_avx2 / svt_av1_highbd_resize_plane_avx2 outputs must equal the C
 * ones (planes with every width >= 32 and every height >= 16: the AVX2 code has no short-input branch; checked after
 * the file is written), or the generator stops.  It also stops unless some extreme record's horizontal stage clips at both ends.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "EbResize.c"
#include "common_dsp_rtcd.h"
#include "golden_io.h"

/* svt_aom_resize_frame's unpacked 10-bit branch (8 + 2 bit planes) is out of scope and never taken here: the frames
 * below are packed 16-bit.  Its helpers live in the encoder's temporal filter and picture operators; stand-ins that stop keep those out. */
void svt_aom_pack_highbd_pic(const EbPictureBufferDesc *pic_ptr, uint16_t *buffer_16bit[3], uint32_t ss_x, uint32_t ss_y,
                             Bool include_padding) {
    (void)pic_ptr, (void)buffer_16bit, (void)ss_x, (void)ss_y, (void)include_padding;
    fprintf(stderr, "unpacked 10-bit path reached\n"), exit(3);
}
void svt_aom_unpack_highbd_pic(uint16_t *buffer_highbd[3], EbPictureBufferDesc *pic_ptr, uint32_t ss_x, uint32_t ss_y,
                               Bool include_padding) {
    (void)pic_ptr, (void)buffer_highbd, (void)ss_x, (void)ss_y, (void)include_padding;
    fprintf(stderr, "unpacked 10-bit path reached\n"), exit(3);
}
void svt_aom_pack2d_src(uint8_t *in8_bit_buffer, uint32_t in8_stride, uint8_t *inn_bit_buffer, uint32_t inn_stride,
                        uint16_t *out16_bit_buffer, uint32_t out_stride, uint32_t width, uint32_t height) {
    (void)in8_bit_buffer, (void)in8_stride, (void)inn_bit_buffer, (void)inn_stride, (void)out16_bit_buffer;
    (void)out_stride, (void)width, (void)height;
    fprintf(stderr, "unpacked 10-bit path reached\n"), exit(3);
}
void svt_aom_un_pack2d(uint16_t *in16_bit_buffer, uint32_t in_stride, uint8_t *out8_bit_buffer, uint32_t out8_stride,
                       uint8_t *outn_bit_buffer, uint32_t outn_stride, uint32_t width, uint32_t height) {
    (void)in16_bit_buffer, (void)in_stride, (void)out8_bit_buffer, (void)out8_stride, (void)outn_bit_buffer;
    (void)outn_stride, (void)width, (void)height;
    fprintf(stderr, "unpacked 10-bit path reached\n"), exit(3);
}

static void bind_c_kernels(void) {
    svt_memcpy                      = svt_memcpy_c;
    svt_av1_interpolate_core        = svt_av1_interpolate_core_c;
    svt_av1_down2_symeven           = svt_av1_down2_symeven_c;
    svt_av1_highbd_interpolate_core = svt_av1_highbd_interpolate_core_c;
    svt_av1_highbd_down2_symeven    = svt_av1_highbd_down2_symeven_c;
    svt_av1_resize_plane            = svt_av1_resize_plane_c; /* svt_aom_resize_frame calls through these two */
    svt_av1_highbd_resize_plane     = svt_av1_highbd_resize_plane_c;
}

static int scaled(int dim, int denom) {
    uint16_t d = (uint16_t)dim;
    calculate_scaled_size_helper(&d, (uint8_t)denom);
    return d;
}

static const InterpKernel *const k_tables[5] = {svt_aom_av1_filteredinterp_filters500, svt_aom_av1_filteredinterp_filters625,
                                                svt_aom_av1_filteredinterp_filters750, svt_aom_av1_filteredinterp_filters875,
                                                filteredinterp_filters1000};

static int table_index(int in_length, int out_length) {
    const InterpKernel *f = choose_interp_filter(in_length, out_length);
    for (int i = 0; i < 5; i++)
        if (f == k_tables[i]) return i;
    fprintf(stderr, "unknown filter table\n");
    exit(3);
}

/* the position step and start of one interpolation, as svt_av1_interpolate_core_c forms them (its locals) */
static void interp_geometry(int in_length, int out_length, int32_t *delta, int32_t *offset) {
    *delta = (int32_t)((((uint32_t)in_length << 14) + out_length / 2) / out_length);
    const int32_t half = ((in_length > out_length ? in_length - out_length : out_length - in_length) << 13) + out_length / 2;
    *offset = in_length > out_length ? half / out_length : -half / out_length;
}

enum { CONTENT_RANDOM, CONTENT_EXTREME };
typedef struct PlaneCase {
    int bd, in_w, in_h, out_w, out_h, content;
} PlaneCase;

static void fill_plane(const PlaneCase *c, Rng *r, uint16_t *src) {
    const int maxv = (1 << c->bd) - 1, w = c->in_w;
    for (int y = 0; y < c->in_h; y++)
        for (int x = 0; x < w; x++) {
            int v;
            if (c->content == CONTENT_RANDOM) {
                v = y & 1 ? (int)rng_below(r, (uint32_t)maxv + 1)
                          : (x * 5 + y * 3) * (maxv + 1) / 512 + (int)rng_below(r, (uint32_t)(maxv / 4 + 1));
                v = v < 0 ? 0 : v > maxv ? maxv : v;
            } else {
                switch (y % 8) {
                case 0: v = x & 1 ? maxv : 0; break;                   /* alternating columns, both phases */
                case 1: v = x & 1 ? 0 : maxv; break;
                case 2: v = (x == 0 || x == 1 || x == 20 || x == w / 2 || x == w - 1) ? maxv : 0; break; /* impulses */
                case 3: v = (x == 0 || x == 1 || x == 20 || x == w / 2 || x == w - 1) ? 0 : maxv; break; /* dips */
                case 4: v = maxv; break;                               /* rows 4 / 5: alternating rows */
                case 5: v = 0; break;
                case 6: v = x & 2 ? 0 : maxv; break;                   /* pairs */
                default: v = (x / 3) & 1 ? maxv : 0; break;            /* triples */
                }
            }
            src[y * w + x] = (uint16_t)v;
        }
}



/* The AVX2 plane functions have no short-input branch: they assert on it, and on 20x20 -> 16x16 they write past their
 * buffers.  They are compared where every width is >= 32 and every height >= 16, after the file is closed. */
static int have_avx2(const PlaneCase *c) {
    return __builtin_cpu_supports("avx2") && c->in_w >= 32 && c->out_w >= 32 && c->in_h >= 16 && c->out_h >= 16;
}

/* one plane through the reference: the function svt_aom_resize_frame would pick; the AVX2 one must agree */
static void run_plane(const PlaneCase *c, const uint16_t *src, uint16_t *out) {
    const int ns = c->in_w * c->in_h, nd = c->out_w * c->out_h;
    if (c->bd > 8) {
        uint16_t *chk = malloc(sizeof(uint16_t) * nd);
        if (c->in_h == c->out_h)
            svt_av1_highbd_resize_plane_horizontal(src, c->in_h, c->in_w, c->in_w, out, c->out_h, c->out_w, c->out_w, c->bd);
        else
            svt_av1_highbd_resize_plane_c(src, c->in_h, c->in_w, c->in_w, out, c->out_h, c->out_w, c->out_w, c->bd);
        /* the general function on equal heights is the same thing (the vertical stage copies) */
        svt_av1_highbd_resize_plane_c(src, c->in_h, c->in_w, c->in_w, chk, c->out_h, c->out_w, c->out_w, c->bd);
        if (memcmp(chk, out, sizeof(uint16_t) * nd)) fprintf(stderr, "horizontal != general\n"), exit(3);
        free(chk);
    } else {
        uint8_t *s8 = malloc(ns), *d8 = malloc(nd), *chk = malloc(nd);
        for (int i = 0; i < ns; i++) s8[i] = (uint8_t)src[i];
        if (c->in_h == c->out_h)
            svt_av1_resize_plane_horizontal(s8, c->in_h, c->in_w, c->in_w, d8, c->out_h, c->out_w, c->out_w);
        else
            svt_av1_resize_plane_c(s8, c->in_h, c->in_w, c->in_w, d8, c->out_h, c->out_w, c->out_w);
        svt_av1_resize_plane_c(s8, c->in_h, c->in_w, c->in_w, chk, c->out_h, c->out_w, c->out_w);
        if (memcmp(chk, d8, nd)) fprintf(stderr, "horizontal != general\n"), exit(3);
        for (int i = 0; i < nd; i++) out[i] = d8[i];
        free(s8), free(d8), free(chk);
    }
}

/* the sums of the horizontal stage before the clip (no halving step): counts those below 0 and above max; the clipped
 * sums must be what the reference's horizontal function gives */
static void count_clipped(const PlaneCase *c, const uint16_t *src, int32_t cnt[2]) {
    cnt[0] = cnt[1] = 0;
    if (c->in_w == c->out_w || get_down2_steps(c->in_w, c->out_w)) return;
    const int      maxv = (1 << c->bd) - 1;
    const int16_t *tab  = &k_tables[table_index(c->in_w, c->out_w)][0][0];
    int32_t        delta, offset;
    interp_geometry(c->in_w, c->out_w, &delta, &offset);
    PlaneCase h = *c;
    h.out_h     = h.in_h;
    uint16_t *ref = malloc(sizeof(uint16_t) * h.out_w * h.out_h);
    run_plane(&h, src, ref);
    for (int y = 0; y < c->in_h; y++)
        for (int x = 0; x < c->out_w; x++) {
            const int32_t pos = offset + 128 + x * delta;
            int           sum = 64;
            for (int k = 0; k < 8; k++) {
                int i = (pos >> 14) - 3 + k;
                i     = i < 0 ? 0 : i > c->in_w - 1 ? c->in_w - 1 : i;
                sum += tab[((pos >> 8) & 63) * 8 + k] * src[y * c->in_w + i];
            }
            sum >>= 7;
            cnt[0] += sum < 0, cnt[1] += sum > maxv;
            if ((sum < 0 ? 0 : sum > maxv ? maxv : sum) != ref[y * c->out_w + x])
                fprintf(stderr, "the clip count's sums disagree with the reference\n"), exit(3);
        }
    free(ref);
}

#define MAXCASES 256
static PlaneCase g_cases[MAXCASES];
static int       g_n;
static void      add(int bd, int in_w, int in_h, int out_w, int out_h, int content) {
    if (g_n == MAXCASES) exit(4);
    g_cases[g_n++] = (PlaneCase){bd, in_w, in_h, out_w, out_h, content};
}

/* The device kernels' tiles (csrc/resize.hip): a wave makes 512 adjacent outputs of a row, a workgroup 4 rows; the
 * vertical kernels' workgroup makes 4 output rows of 512 columns.  tests/test_resize_gpu.py names the same numbers. */
#define TILE_W 512
#define TILE_ROWS 4

static void list_cases(void) {
    for (int bd = 8; bd <= 10; bd += 2) {
        for (int denom = 9; denom <= 17; denom++) { /* luma 88x16 and its chroma 44x8 */
            add(bd, 88, 16, scaled(88, denom), scaled(16, denom), CONTENT_RANDOM);
            add(bd, 44, 8, (scaled(88, denom) + 1) >> 1, (scaled(16, denom) + 1) >> 1, CONTENT_RANDOM);
        }
        add(bd, 83, 17, 42, 9, CONTENT_RANDOM);   /* odd lengths: symodd in both directions */
        add(bd, 83, 17, 61, 13, CONTENT_RANDOM);
        add(bd, 88, 16, 66, 16, CONTENT_RANDOM);  /* width only */
        add(bd, 88, 16, 44, 16, CONTENT_RANDOM);
        add(bd, 88, 16, 88, 12, CONTENT_RANDOM);  /* height only */
        add(bd, 88, 17, 88, 9, CONTENT_RANDOM);
        add(bd, 44, 8, 88, 16, CONTENT_RANDOM);   /* upscales: the normative table */
        add(bd, 45, 9, 67, 16, CONTENT_RANDOM);
        add(bd, 40, 100, 22, 55, CONTENT_RANDOM); /* the 0.5-band table in both directions */
        add(bd, 24, 40, 15, 25, CONTENT_RANDOM);  /* the 0.625-band table in both directions */
        add(bd, 100, 40, 25, 10, CONTENT_RANDOM); /* two halving steps, nothing after them */
        add(bd, 100, 40, 23, 9, CONTENT_RANDOM);  /* two steps and an interpolation */
        add(bd, 130, 8, 17, 8, CONTENT_RANDOM);   /* three steps (130, 65, 33, 17), width only */
        add(bd, 8, 131, 8, 15, CONTENT_RANDOM);   /* three steps and an interpolation, height only */
        add(bd, 5, 5, 3, 3, CONTENT_RANDOM);      /* the short-input branches */
        add(bd, 7, 7, 4, 4, CONTENT_RANDOM);
        add(bd, 3, 3, 2, 2, CONTENT_RANDOM);
        add(bd, 2, 2, 1, 1, CONTENT_RANDOM);
        add(bd, 7, 3, 5, 2, CONTENT_RANDOM);
        add(bd, 9, 6, 8, 5, CONTENT_RANDOM);
        add(bd, 20, 20, 16, 16, CONTENT_RANDOM);  /* the min(16, dim) floor of denominators 11..16 */
        add(bd, 88, 16, scaled(88, 11), scaled(16, 11), CONTENT_EXTREME);
        add(bd, 88, 16, scaled(88, 13), scaled(16, 13), CONTENT_EXTREME);
        add(bd, 88, 16, scaled(88, 15), scaled(16, 15), CONTENT_EXTREME);
        add(bd, 88, 16, 66, 12, CONTENT_EXTREME);
        add(bd, 88, 16, 44, 8, CONTENT_EXTREME);
        add(bd, 83, 17, 42, 9, CONTENT_EXTREME);
        add(bd, 44, 8, 88, 16, CONTENT_EXTREME);
    }
    /* tile seams: outputs one sample short of and one past two tiles, in each direction, by interpolation and halving */
    add(8, 1364, 3, 2 * TILE_W - 1, 3, CONTENT_RANDOM);
    add(10, 1367, 5, 2 * TILE_W + 1, 4, CONTENT_RANDOM);
    add(10, 4 * TILE_W - 2, 3, 2 * TILE_W - 1, 3, CONTENT_RANDOM);
    add(8, 4 * TILE_W + 2, 3, 2 * TILE_W + 1, 2, CONTENT_RANDOM);
    add(10, 5, 800, 5, 150 * TILE_ROWS - 1, CONTENT_RANDOM);
    add(8, 7, 801, 6, 150 * TILE_ROWS + 1, CONTENT_RANDOM);
    add(8, 3, 300 * TILE_ROWS - 2, 3, 150 * TILE_ROWS - 1, CONTENT_RANDOM);
    add(10, 3, 300 * TILE_ROWS + 2, 3, 150 * TILE_ROWS + 1, CONTENT_RANDOM);
    add(10, TILE_W + 9, 6, TILE_W + 1, 5, CONTENT_RANDOM); /* the vertical kernel's second column tile */
    add(10, 3840, 2, 2880, 2, CONTENT_RANDOM); /* wide rows */
}

static void put_plane(GoldenFile *g, const char *nm, int bd, int h, int w, const uint16_t *a) {
    if (bd > 8) {
        golden_put2(g, nm, 'H', (uint32_t)h, (uint32_t)w, a);
        return;
    }
    uint8_t *b = malloc((size_t)w * h);
    for (int i = 0; i < w * h; i++) b[i] = (uint8_t)a[i];
    golden_put2(g, nm, 'B', (uint32_t)h, (uint32_t)w, b);
    free(b);
}

static void gen_tables(GoldenFile *g) {
    int16_t half[2][4];
    memcpy(half[0], svt_aom_av1_down2_symeven_half_filter, sizeof half[0]);
    memcpy(half[1], av1_down2_symodd_half_filter, sizeof half[1]);
    int16_t(*f)[64][8] = malloc(sizeof(int16_t) * 5 * 64 * 8);
    for (int i = 0; i < 5; i++) memcpy(f[i], k_tables[i], sizeof f[i]);
    uint32_t d[3] = {5, 64, 8};
    golden_put(g, "filters", 'h', 3, d, f);
    golden_put2(g, "half_filters", 'h', 2, 4, half);
    free(f);

    static const int pairs[][2] = {{88, 78}, {88, 70}, {88, 64}, {88, 59}, {88, 54}, {88, 50}, {88, 47}, {88, 44},
                                   {88, 66}, {16, 14}, {16, 12}, {16, 8},  {44, 39}, {44, 33}, {44, 22}, {83, 42},
                                   {17, 9},  {83, 61}, {100, 25}, {100, 23}, {40, 10}, {40, 9}, {130, 17}, {131, 15},
                                   {5, 3},   {7, 4},   {3, 2},   {2, 1},   {3, 1},   {1, 1},   {1, 2},   {9, 8},
                                   {20, 16}, {44, 88}, {45, 67}, {8, 16},  {9, 16},  {3840, 2880}, {3840, 1920},
                                   {3840, 2560}, {2160, 1620}, {3840, 960}, {3840, 961}, {65535, 4097}, {4096, 8192}};
    const int     n = (int)(sizeof pairs / sizeof pairs[0]);
    int32_t(*p)[7] = calloc((size_t)n, sizeof *p);
    for (int i = 0; i < n; i++) {
        const int in = pairs[i][0], out = pairs[i][1];
        p[i][0] = in, p[i][1] = out, p[i][4] = -1;
        p[i][2] = in == out ? 0 : get_down2_steps(in, out);
        p[i][3] = get_down2_length(in, p[i][2]);
        if (p[i][3] != out) {
            p[i][4] = table_index(p[i][3], out);
            interp_geometry(p[i][3], out, &p[i][5], &p[i][6]);
        }
    }
    golden_put2(g, "plan", 'i', (uint32_t)n, 7, p);
    free(p);
    int32_t sc[9][4];
    for (int d2 = 9; d2 <= 17; d2++)
        sc[d2 - 9][0] = d2, sc[d2 - 9][1] = scaled(88, d2), sc[d2 - 9][2] = scaled(16, d2), sc[d2 - 9][3] = scaled(44, d2);
    golden_put2(g, "scaled", 'i', 9, 4, sc);
}

static void gen_planes(GoldenFile *g) {
    Rng     r  = {0x5253000000000001ull};
    int32_t np = g_n, both = 0;
    int32_t(*clipped)[2] = calloc((size_t)g_n, sizeof *clipped);
    golden_put1(g, "nplane", 'i', 1, &np);
    for (int i = 0; i < g_n; i++) {
        const PlaneCase *c   = &g_cases[i];
        uint16_t        *src = malloc(sizeof(uint16_t) * c->in_w * c->in_h);
        uint16_t        *out = malloc(sizeof(uint16_t) * c->out_w * c->out_h);
        fill_plane(c, &r, src);
        run_plane(c, src, out);
        if (c->content == CONTENT_EXTREME) {
            count_clipped(c, src, clipped[i]);
            both += clipped[i][0] > 0 && clipped[i][1] > 0;
        }
        int32_t par[6] = {c->bd, c->in_w, c->in_h, c->out_w, c->out_h, c->content};
        char    nm[32];
        snprintf(nm, sizeof nm, "p%d_par", i);
        golden_put1(g, nm, 'i', 6, par);
        snprintf(nm, sizeof nm, "p%d_src", i);
        put_plane(g, nm, c->bd, c->in_h, c->in_w, src);
        snprintf(nm, sizeof nm, "p%d_out", i);
        put_plane(g, nm, c->bd, c->out_h, c->out_w, out);
        free(src), free(out);
    }
    if (!both) fprintf(stderr, "no extreme record clips at both ends\n"), exit(3);
    golden_put2(g, "clipped", 'i', (uint32_t)g_n, 2, clipped);
    free(clipped);
}

/* the same planes again (the same input stream) through the reference's AVX2 functions */
static int check_avx2(void) {
    Rng r = {0x5253000000000001ull};
    int n = 0;
    for (int i = 0; i < g_n; i++) {
        const PlaneCase *c   = &g_cases[i];
        const int        ns = c->in_w * c->in_h, nd = c->out_w * c->out_h;
        uint16_t        *src = malloc(sizeof(uint16_t) * ns), *out = malloc(sizeof(uint16_t) * nd);
        uint16_t        *chk = malloc(sizeof(uint16_t) * nd);
        fill_plane(c, &r, src);
        if (have_avx2(c)) {
            run_plane(c, src, out);
            if (c->bd > 8) {
                svt_av1_highbd_resize_plane_avx2(src, c->in_h, c->in_w, c->in_w, chk, c->out_h, c->out_w, c->out_w, c->bd);
            } else {
                uint8_t *s8 = malloc(ns), *d8 = malloc(nd);
                for (int k = 0; k < ns; k++) s8[k] = (uint8_t)src[k];
                svt_av1_resize_plane_avx2(s8, c->in_h, c->in_w, c->in_w, d8, c->out_h, c->out_w, c->out_w);
                for (int k = 0; k < nd; k++) chk[k] = d8[k];
                free(s8), free(d8);
            }
            if (memcmp(chk, out, sizeof(uint16_t) * nd)) {
                fprintf(stderr, "avx2 != c: case %d, %d-bit %dx%d -> %dx%d\n", i, c->bd, c->in_w, c->in_h, c->out_w, c->out_h);
                exit(3);
            }
            n++;
        }
        free(src), free(out), free(chk);
    }
    return n;
}

/* ---- whole frames through svt_aom_resize_frame ---- */
#define PAD 8
static void desc_init(EbPictureBufferDesc *d, int w, int h, int bd) {
    memset(d, 0, sizeof *d);
    const int bs = bd > 8 ? 2 : 1, cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    d->width = (uint16_t)w, d->height = (uint16_t)h, d->max_width = (uint16_t)w, d->max_height = (uint16_t)h;
    d->org_x = d->org_y = d->origin_bot_y = PAD;
    d->stride_y  = (uint16_t)(w + 2 * PAD);
    d->stride_cb = d->stride_cr = (uint16_t)(cw + 2 * PAD);
    d->luma_size   = (uint32_t)(d->stride_y * (h + 2 * PAD));
    d->chroma_size = (uint32_t)(d->stride_cb * (ch + 2 * PAD));
    d->buffer_y    = calloc(d->luma_size, bs);
    d->buffer_cb   = calloc(d->chroma_size, bs);
    d->buffer_cr   = calloc(d->chroma_size, bs);
    d->bit_depth   = bd > 8 ? EB_SIXTEEN_BIT : EB_EIGHT_BIT;
    d->is_16bit_pipeline = bd > 8;
}
static uint8_t *desc_plane(const EbPictureBufferDesc *d, int p, int *stride, int *ox, int *oy) {
    *stride = p == 0 ? d->stride_y : p == 1 ? d->stride_cb : d->stride_cr;
    *ox = p ? d->org_x >> 1 : d->org_x, *oy = p ? d->org_y >> 1 : d->org_y;
    return p == 0 ? d->buffer_y : p == 1 ? d->buffer_cb : d->buffer_cr;
}
static void desc_free(EbPictureBufferDesc *d) { free(d->buffer_y), free(d->buffer_cb), free(d->buffer_cr); }

static void gen_frames(GoldenFile *g) {
    static const int cases[][5] = {{8, 120, 72, 90, 54},   /* code 17 */
                                   {10, 104, 58, 52, 29},  /* packed 10-bit, denominator 16: one halving step each way */
                                   {10, 99, 45, 71, 45},   /* odd sizes, width only: the _horizontal functions */
                                   {8, 50, 30, 75, 45}};   /* an upscale */
    const int        n = (int)(sizeof cases / sizeof cases[0]);
    int32_t          nf = n;
    Rng              r  = {0x5253000000000002ull};
    golden_put1(g, "nframe", 'i', 1, &nf);
    for (int i = 0; i < n; i++) {
        const int bd = cases[i][0], sw = cases[i][1], sh = cases[i][2], dw = cases[i][3], dh = cases[i][4];
        const int maxv = (1 << bd) - 1;
        EbPictureBufferDesc s, d;
        desc_init(&s, sw, sh, bd);
        desc_init(&d, dw, dh, bd);
        int32_t par[5] = {bd, sw, sh, dw, dh};
        char    nm[32];
        snprintf(nm, sizeof nm, "f%d_par", i);
        golden_put1(g, nm, 'i', 5, par);
        for (int p = 0; p < 3; p++) {
            int       st, ox, oy;
            uint8_t  *b = desc_plane(&s, p, &st, &ox, &oy);
            const int w = p ? (sw + 1) >> 1 : sw, h = p ? (sh + 1) >> 1 : sh;
            uint16_t *a = malloc(sizeof(uint16_t) * w * h);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    int v = (x * 7 + y * 5) * (maxv + 1) / 640 + (int)rng_below(&r, (uint32_t)(maxv / 3 + 1));
                    v     = v > maxv ? maxv : v;
                    a[y * w + x] = (uint16_t)v;
                    if (bd > 8)
                        ((uint16_t *)b)[(y + oy) * st + x + ox] = (uint16_t)v;
                    else
                        b[(y + oy) * st + x + ox] = (uint8_t)v;
                }
            snprintf(nm, sizeof nm, "f%d_src%d", i, p);
            put_plane(g, nm, bd, h, w, a);
            free(a);
        }
        if (svt_aom_resize_frame(&s, &d, bd, 3, 1, 1, bd > 8, PICTURE_BUFFER_DESC_FULL_MASK, 0) != EB_ErrorNone) exit(3);
        for (int p = 0; p < 3; p++) {
            int       st, ox, oy;
            uint8_t  *b = desc_plane(&d, p, &st, &ox, &oy);
            const int w = p ? (dw + 1) >> 1 : dw, h = p ? (dh + 1) >> 1 : dh;
            uint16_t *a = malloc(sizeof(uint16_t) * w * h);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    a[y * w + x] = bd > 8 ? ((uint16_t *)b)[(y + oy) * st + x + ox] : b[(y + oy) * st + x + ox];
            snprintf(nm, sizeof nm, "f%d_out%d", i, p);
            put_plane(g, nm, bd, h, w, a);
            free(a);
        }
        desc_free(&s), desc_free(&d);
    }
}

/* scripts/resize_perf.py's workloads (10-bit 4:2:0, three planes) through the reference's C on one core */
static void time_reference(void) {
    static const int shapes[3][4] = {{3840, 2160, 2880, 1620}, {3840, 2160, 1920, 1080}, {3840, 2160, 2560, 2160}};
    Rng              r            = {0x5253000000000003ull};
    for (int k = 0; k < 3; k++) {
        const int sw = shapes[k][0], sh = shapes[k][1], dw = shapes[k][2], dh = shapes[k][3];
        uint16_t *src[3], *dst[3];
        for (int p = 0; p < 3; p++) {
            const int s = p > 0;
            src[p]      = malloc(sizeof(uint16_t) * (sw >> s) * (sh >> s));
            dst[p]      = malloc(sizeof(uint16_t) * (dw >> s) * (dh >> s));
            for (int i = 0; i < (sw >> s) * (sh >> s); i++) src[p][i] = (uint16_t)rng_below(&r, 1024);
        }
        double   best = 1e30;
        uint64_t sum  = 0;
        for (int rep = 0; rep < 3; rep++) {
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            for (int p = 0; p < 3; p++) {
                const int s = p > 0;
                (sh == dh ? svt_av1_highbd_resize_plane_horizontal : svt_av1_highbd_resize_plane_c)(
                    src[p], sh >> s, sw >> s, sw >> s, dst[p], dh >> s, dw >> s, dw >> s, 10);
            }
            clock_gettime(CLOCK_MONOTONIC, &t1);
            const double ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
            if (ms < best) best = ms;
        }
        for (int p = 0; p < 3; p++) {
            for (int i = 0; i < (dw >> (p > 0)) * (dh >> (p > 0)); i += 97) sum += dst[p][i];
            free(src[p]), free(dst[p]);
        }
        printf("{\"workload\": \"%dx%d -> %dx%d 10-bit, three planes\", \"reference_c_ms\": %.2f, \"reps\": 3, "
               "\"sample_sum\": %llu}\n", sw, sh, dw, dh, best, (unsigned long long)sum);
    }
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
    list_cases();
    gen_tables(&g);
    gen_planes(&g);
    gen_frames(&g);
    golden_close(&g);
    fprintf(stderr, "%d planes, %d of them equal through the AVX2 functions\n", g_n, check_avx2());
    return 0;
}
