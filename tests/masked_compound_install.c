/*
 * masked_compound_install.c — svtgpu_install_masked_compound_rtcd() against the reference's own RTCD declarations and its
 * complete ConvolveParams (tests/test_masked_compound_rtcd.py; pointer comparisons only, no device call).  Compiled with
 * -Werror=incompatible-pointer-types: the three assignments of include/svtgpu_rtcd.h need no cast, because the adapters carry
 * the reference's prototypes.
 * Output: "before <shims>/3 after <shims>/3".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_MASKED_COMPOUND
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < 3; k++) n += svtgpu_masked_compound_rtcd_bound(k);
    return n;
}

int main(void) {
    /* the three pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_masked_compound_rtcd();
    printf("before %d/3 after %d/3\n", before, shims());
    return 0;
}
