/*
 * obmc_bind.c — compile-only check (tests/test_obmc.py): every OBMC shim prototype of include/svtgpu.h assigns to the
 * reference's RTCD pointer of the same name without a cast.  Built with -fsyntax-only
 * -Werror=incompatible-pointer-types -Werror=discarded-qualifiers against the reference's headers.
 */
#include "EbDefinitions.h"
#include "aom_dsp_rtcd.h"
#include "common_dsp_rtcd.h"
#include "EbMcp.h"
#include "svtgpu_rtcd.h"

void obmc_bind(void) { svtgpu_install_obmc_rtcd(); }
