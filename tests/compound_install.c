/*
 * compound_install.c — svtgpu_install_compound_rtcd() against the reference's own RTCD declarations and its complete
 * InterpFilterParams / ConvolveParams (tests/test_compound_rtcd.py; pointer comparisons only, no device call).  Compiled
 * with -Werror=incompatible-pointer-types: the eight assignments of include/svtgpu_rtcd.h need no cast, because the
 * adapters carry the reference's prototypes (AomConvolveFn, aom_highbd_convolve_fn_t).
 * Output: "before <shims>/8 after <shims>/8".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_COMPOUND
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < 8; k++) n += svtgpu_compound_rtcd_bound(k);
    return n;
}

int main(void) {
    /* the eight pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_compound_rtcd();
    printf("before %d/8 after %d/8\n", before, shims());
    return 0;
}
