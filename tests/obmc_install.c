/*
 * obmc_install.c — the install point of the OBMC shims (tests/test_obmc.py; pointer comparisons only, no device call).
 *
 * init_fn_ptr (av1me.c:31) copies the 66 OBMC pointers into svt_aom_mefn_ptr[].osdf / ovf / osvf (av1me.c:171-196).
 * Linked with the reference's own av1me.c and libsvtgpu, this runs svtgpu_install_obmc_rtcd() on both sides of it:
 *   documented order: install, then init_fn_ptr  -> every entry is a libsvtgpu symbol;
 *   late install:     init_fn_ptr, then install  -> none is.
 * Output: one line "documented <shims>/<entries> late <shims>/<entries>".
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "EbMcp.h"
#include "av1me.h"
#include "svtgpu_rtcd.h"

void init_fn_ptr(void);

static int in_libsvtgpu(const void *f) {
    Dl_info d;
    return f && dladdr(f, &d) && d.dli_fname && strstr(d.dli_fname, "libsvtgpu") != NULL;
}

static void census(int *shims, int *entries) {
    *shims = *entries = 0;
    for (int b = 0; b < BlockSizeS_ALL; b++) {
        const void *f[3] = {(const void *)svt_aom_mefn_ptr[b].osdf, (const void *)svt_aom_mefn_ptr[b].ovf,
                            (const void *)svt_aom_mefn_ptr[b].osvf};
        for (int k = 0; k < 3; k++)
            if (f[k]) ++*entries, *shims += in_libsvtgpu(f[k]);
    }
}

/* stand-ins for what the RTCD setup binds: any function of this program, that is, not one of libsvtgpu's */
static unsigned int host_sad(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask) {
    (void)pre, (void)pre_stride, (void)wsrc, (void)mask;
    return 0;
}
static unsigned int host_var(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask,
                             unsigned int *sse) {
    (void)pre, (void)pre_stride, (void)wsrc, (void)mask, (void)sse;
    return 0;
}
static unsigned int host_subvar(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc,
                                const int32_t *mask, unsigned int *sse) {
    (void)pre, (void)pre_stride, (void)xoffset, (void)yoffset, (void)wsrc, (void)mask, (void)sse;
    return 0;
}
#define HOST_SIZE(w, h)                                      \
    svt_aom_obmc_sad##w##x##h                = host_sad;     \
    svt_aom_obmc_variance##w##x##h           = host_var;     \
    svt_aom_obmc_sub_pixel_variance##w##x##h = host_subvar;
static void bind_host(void) {
    HOST_SIZE(4, 4) HOST_SIZE(4, 8) HOST_SIZE(4, 16) HOST_SIZE(8, 4) HOST_SIZE(8, 8) HOST_SIZE(8, 16) HOST_SIZE(8, 32)
    HOST_SIZE(16, 4) HOST_SIZE(16, 8) HOST_SIZE(16, 16) HOST_SIZE(16, 32) HOST_SIZE(16, 64) HOST_SIZE(32, 8)
    HOST_SIZE(32, 16) HOST_SIZE(32, 32) HOST_SIZE(32, 64) HOST_SIZE(64, 16) HOST_SIZE(64, 32) HOST_SIZE(64, 64)
    HOST_SIZE(64, 128) HOST_SIZE(128, 64) HOST_SIZE(128, 128)
}

int main(void) {
    int s1, e1, s2, e2;
    bind_host();
    svtgpu_install_obmc_rtcd();
    init_fn_ptr();
    census(&s1, &e1);
    bind_host();
    init_fn_ptr();
    svtgpu_install_obmc_rtcd();
    census(&s2, &e2);
    printf("documented %d/%d late %d/%d\n", s1, e1, s2, e2);
    return 0;
}
