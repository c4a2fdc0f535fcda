/*
 * obmc_blend_install.c — svtgpu_install_obmc_blend_rtcd() against the reference's own RTCD declarations
 * (tests/test_obmc_blend_rtcd.py; pointer comparisons only, no device call).  Compiled with
 * -Werror=incompatible-pointer-types: the six assignments of include/svtgpu_rtcd.h need no cast, because the adapters carry the
 * reference's prototypes.
 * Output: "before <shims>/6 after <shims>/6".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_OBMC_BLEND
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < 6; k++) n += svtgpu_obmc_blend_rtcd_bound(k);
    return n;
}

int main(void) {
    /* the six pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_obmc_blend_rtcd();
    printf("before %d/6 after %d/6\n", before, shims());
    return 0;
}
