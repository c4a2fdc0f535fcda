/*
 * warp_install.c — svtgpu_install_warp_rtcd() against the reference's own RTCD declarations and its
 * complete ConvolveParams (tests/test_warp_rtcd.py; pointer comparisons only, no device call).  Compiled with
 * -Werror=incompatible-pointer-types: the two assignments of include/svtgpu_rtcd.h need no cast, because the adapters carry
 * the reference's prototypes.
 * Output: "before <shims>/2 after <shims>/2".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_WARP
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < 2; k++) n += svtgpu_warp_rtcd_bound(k);
    return n;
}

int main(void) {
    /* the two pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_warp_rtcd();
    printf("before %d/2 after %d/2\n", before, shims());
    return 0;
}
