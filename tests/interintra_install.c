/*
 * interintra_install.c — svtgpu_install_interintra_rtcd() against the reference's own RTCD declarations
 * (tests/test_interintra_rtcd.py; pointer comparisons only, no device call).  Compiled with
 * -Werror=incompatible-pointer-types: the 142 assignments of include/svtgpu_rtcd.h need no cast, because the adapters carry the
 * reference's prototypes.
 * Output: "before <shims>/142 after <shims>/142".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "convolve.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_INTERINTRA
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < SVTGPU_INTERINTRA_RTCD_COUNT; k++) n += svtgpu_interintra_rtcd_bound(k);
    return n;
}

int main(void) {
    /* the pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_interintra_rtcd();
    printf("before %d/%d after %d/%d\n", before, SVTGPU_INTERINTRA_RTCD_COUNT, shims(), SVTGPU_INTERINTRA_RTCD_COUNT);
    return svtgpu_interintra_rtcd_bound(SVTGPU_INTERINTRA_RTCD_COUNT) || svtgpu_interintra_rtcd_bound(-1);
}
