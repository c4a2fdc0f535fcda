/*
 * resize_install.c — svtgpu_install_resize_rtcd() against the reference's own RTCD declarations (tests/test_resize.py::test_resize_install_sets_both_plane_pointers;
 * pointer comparisons only, no device call).  Compiled with -Werror=incompatible-pointer-types: the two assignments of
 * include/svtgpu_rtcd.h need no cast because the shims carry the reference's prototypes (SVTGPU_ERROR_T = EbErrorType).
 * Output: "before <shims>/2 after <shims>/2".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "EbMcp.h"
#include "svtgpu_rtcd.h"

/* stand-ins for what the RTCD setup binds: functions of this program, that is, not libsvtgpu's */
static EbErrorType host_plane(const uint8_t *const input, int height, int width, int in_stride, uint8_t *output,
                              int height2, int width2, int out_stride) {
    (void)input, (void)height, (void)width, (void)in_stride, (void)output, (void)height2, (void)width2, (void)out_stride;
    return EB_ErrorNone;
}
static EbErrorType host_plane_highbd(const uint16_t *const input, int height, int width, int in_stride, uint16_t *output,
                                     int height2, int width2, int out_stride, int bd) {
    (void)input, (void)height, (void)width, (void)in_stride, (void)output, (void)height2, (void)width2, (void)out_stride;
    (void)bd;
    return EB_ErrorNone;
}

static int shims(void) {
    return (svt_av1_resize_plane == svtgpu_av1_resize_plane) + (svt_av1_highbd_resize_plane == svtgpu_av1_highbd_resize_plane);
}

int main(void) {
    svt_av1_resize_plane        = host_plane;
    svt_av1_highbd_resize_plane = host_plane_highbd;
    const int before            = shims();
    svtgpu_install_resize_rtcd();
    printf("before %d/2 after %d/2\n", before, shims());
    return 0;
}
