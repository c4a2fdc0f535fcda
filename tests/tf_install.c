/*
 * tf_install.c — svtgpu_install_tf_rtcd() against the reference's own RTCD declarations and its complete MeContext /
 * EbPictureBufferDesc (tests/test_tf.py::test_tf_install_sets_all_nine_pointers; pointer comparisons only, no device
 * call).  Compiled with -Werror=incompatible-pointer-types: the nine assignments of include/svtgpu_rtcd.h need no cast,
 * because the adapters carry the reference's prototypes and the two noise shims are exported with them.
 * Output: "before <shims>/9 after <shims>/9".
 */
#include <stdio.h>

#include "EbDefinitions.h"
#include "EbPictureBufferDesc.h"
#include "EbMotionEstimationContext.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "EbMcp.h"
#define SVTGPU_RTCD_WITH_TF
#include "svtgpu_rtcd.h"

static int shims(void) {
    int n = 0;
    for (int k = 0; k < 9; k++) n += svtgpu_tf_rtcd_installed(k);
    return n;
}

int main(void) {
    /* the nine pointers are null until an RTCD setup or an install binds them */
    const int before = shims();
    svtgpu_install_tf_rtcd();
    printf("before %d/9 after %d/9\n", before, shims());
    return 0;
}
