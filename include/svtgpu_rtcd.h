/*
 * svtgpu_rtcd.h — installs libsvtgpu's per-block shims into the SVT-AV1 encoder's RTCD function pointers.
 *
 * Include it in ONE translation unit of the encoder that sees the reference's RTCD declarations (common_dsp_rtcd.h,
 * aom_dsp_rtcd.h, EbMcp.h) and call the install functions between the RTCD setup and the first copy of those pointers:
 *
 *     svt_aom_setup_common_rtcd_internal(...);            // EbEncHandle.c:1530
 *     svt_aom_setup_rtcd_internal(...);                   // EbEncHandle.c:1531 (SET_FUNCTIONS may set a pointer once,
 *                                                         //   aom_dsp_rtcd.c:56-68, so install after it)
 *     if (getenv("SVT_GPU") && svtgpu_device_available()) {
 *         svtgpu_install_filter_rtcd();                   // the in-loop filter path (DLF / CDEF / LR)
 *         svtgpu_install_me_md_rtcd();                    // ME / MD distortion + frame buffers
 *         svtgpu_install_ccso_rtcd();                     // CCSO's block kernels (an encoder that re-enables it)
 *         svtgpu_install_obmc_rtcd();                     // OBMC sad / variance / sub-pixel variance (osdf / ovf / osvf)
 *         svtgpu_install_resize_rtcd();                   // svt_av1_resize_plane / svt_av1_highbd_resize_plane
 *         svtgpu_install_tf_rtcd();                       // the temporal filter's nine pointers (define
 *                                                         //   SVTGPU_RTCD_WITH_TF before including this header)
 *         svtgpu_install_obmc_blend_rtcd();               // the six OBMC blends (define SVTGPU_RTCD_WITH_OBMC_BLEND)
 *         svtgpu_install_masked_compound_rtcd();          // the DIFFWTD mask and the two blend_a64_d16_mask (define
 *                                                         // SVTGPU_RTCD_WITH_MASKED_COMPOUND first)
 *         svtgpu_install_warp_rtcd();                     // svt_av1_warp_affine / svt_av1_highbd_warp_affine (define
 *                                                         //   SVTGPU_RTCD_WITH_WARP first)
 *         svtgpu_install_compound_rtcd();                 // the eight compound (jnt_) convolves (define
 *                                                         //   SVTGPU_RTCD_WITH_COMPOUND); same install point as the next
 *         svtgpu_install_interp_rtcd();                   // the eight single-reference convolves (define
 *                                                         //   SVTGPU_RTCD_WITH_INTERP); must precede
 *                                                         //   svt_aom_asm_set_convolve_asm_table(), :1533, which copies them
 *     }
 *     ...
 *     init_fn_ptr();                                      // EbEncHandle.c:1546: av1me.c:31 COPIES the sad / variance /
 *                                                         //   sub-pixel variance / x4d pointers into svt_aom_mefn_ptr[],
 *                                                         //   which MD and ME call (EbProductCodingLoop.c:999, ...);
 *                                                         //   an install after this line leaves those calls on the CPU
 *
 * (tests/test_rtcd_bind.py: oracle/_ref/rtcd_install runs this order against the reference's own init_fn_ptr and
 * checks every svt_aom_mefn_ptr[] entry, and the opposite order.)
 *
 * Every shim prototype names the reference's own types through the type hooks of svtgpu.h, so each assignment below
 * compiles under -Werror=incompatible-pointer-types without a cast.  The shims are synchronous per-block entry points
 * (the reference's unit tests run against the device through them); the fast path is the frame-level API.
 */
#ifndef SVTGPU_RTCD_H
#define SVTGPU_RTCD_H
#ifndef SVTGPU_CDEF_LIST_T
#define SVTGPU_CDEF_LIST_T CdefList
#endif
#ifndef SVTGPU_BLOCK_SIZE_T
#define SVTGPU_BLOCK_SIZE_T BlockSize
#endif
#ifndef SVTGPU_SGR_PARAMS_T
#define SVTGPU_SGR_PARAMS_T SgrParamsType
#endif
#ifndef SVTGPU_CONVOLVE_PARAMS_T
#define SVTGPU_CONVOLVE_PARAMS_T ConvolveParams
#endif
#ifndef SVTGPU_BIT_DEPTH_T
#define SVTGPU_BIT_DEPTH_T EbBitDepth
#endif
#ifndef SVTGPU_ERROR_T
#define SVTGPU_ERROR_T EbErrorType
#endif
#include "svtgpu.h"

/* the in-loop filter path: loop filter x16, CDEF, Wiener / self-guided filters and statistics, the full-distortion
 * kernels (common_dsp_rtcd.h, aom_dsp_rtcd.h) */
static inline void svtgpu_install_filter_rtcd(void) {
    svt_aom_lpf_horizontal_4               = svtgpu_lpf_horizontal_4;
    svt_aom_lpf_horizontal_6               = svtgpu_lpf_horizontal_6;
    svt_aom_lpf_horizontal_8               = svtgpu_lpf_horizontal_8;
    svt_aom_lpf_horizontal_14              = svtgpu_lpf_horizontal_14;
    svt_aom_lpf_vertical_4                 = svtgpu_lpf_vertical_4;
    svt_aom_lpf_vertical_6                 = svtgpu_lpf_vertical_6;
    svt_aom_lpf_vertical_8                 = svtgpu_lpf_vertical_8;
    svt_aom_lpf_vertical_14                = svtgpu_lpf_vertical_14;
    svt_aom_highbd_lpf_horizontal_4        = svtgpu_highbd_lpf_horizontal_4;
    svt_aom_highbd_lpf_horizontal_6        = svtgpu_highbd_lpf_horizontal_6;
    svt_aom_highbd_lpf_horizontal_8        = svtgpu_highbd_lpf_horizontal_8;
    svt_aom_highbd_lpf_horizontal_14       = svtgpu_highbd_lpf_horizontal_14;
    svt_aom_highbd_lpf_vertical_4          = svtgpu_highbd_lpf_vertical_4;
    svt_aom_highbd_lpf_vertical_6          = svtgpu_highbd_lpf_vertical_6;
    svt_aom_highbd_lpf_vertical_8          = svtgpu_highbd_lpf_vertical_8;
    svt_aom_highbd_lpf_vertical_14         = svtgpu_highbd_lpf_vertical_14;
    svt_spatial_full_distortion_kernel     = svtgpu_spatial_full_distortion_kernel;
    svt_full_distortion_kernel16_bits      = svtgpu_full_distortion_kernel16_bits;
    svt_cdef_filter_block                  = svtgpu_cdef_filter_block;
    svt_cdef_filter_block_8xn_16           = svtgpu_cdef_filter_block_8xn_16;
    svt_aom_cdef_find_dir                  = svtgpu_cdef_find_dir;
    svt_aom_cdef_find_dir_dual             = svtgpu_cdef_find_dir_dual;
    svt_compute_cdef_dist_16bit            = svtgpu_compute_cdef_dist_16bit;
    svt_compute_cdef_dist_8bit             = svtgpu_compute_cdef_dist_8bit;
    svt_search_one_dual                    = svtgpu_search_one_dual;
    svt_aom_copy_rect8_8bit_to_16bit       = svtgpu_aom_copy_rect8_8bit_to_16bit;
    svt_av1_wiener_convolve_add_src        = svtgpu_av1_wiener_convolve_add_src;
    svt_av1_highbd_wiener_convolve_add_src = svtgpu_av1_highbd_wiener_convolve_add_src;
    svt_av1_selfguided_restoration         = svtgpu_av1_selfguided_restoration;
    svt_apply_selfguided_restoration       = svtgpu_apply_selfguided_restoration;
    svt_av1_compute_stats                  = svtgpu_av1_compute_stats;
    svt_av1_compute_stats_highbd           = svtgpu_av1_compute_stats_highbd;
    svt_get_proj_subspace                  = svtgpu_get_proj_subspace;
    svt_av1_lowbd_pixel_proj_error         = svtgpu_av1_lowbd_pixel_proj_error;
    svt_av1_highbd_pixel_proj_error        = svtgpu_av1_highbd_pixel_proj_error;
    svt_aom_mse16x16                       = svtgpu_aom_mse16x16;
    svt_aom_highbd_8_mse16x16              = svtgpu_aom_highbd_8_mse16x16;
}

/* CCSO's per-block kernels (common_dsp_rtcd.h:1025-1090), for an encoder that re-enables the fork's CCSO search /
 * apply (EbCdefProcess.c:621-623); the frame-level path is svtgpu_ccso_search_frame + svtgpu_ccso_apply_plane */
static inline void svtgpu_install_ccso_rtcd(void) {
    ccso_filter_block_hbd_wo_buf   = svtgpu_ccso_filter_block_hbd_wo_buf;
    ccso_filter_block_hbd_with_buf = svtgpu_ccso_filter_block_hbd_with_buf;
    ccso_derive_src_block          = svtgpu_ccso_derive_src_block;
    compute_distortion_block       = svtgpu_compute_distortion_block;
}

/* ME and MD distortion (every SAD / x4d / variance / highbd variance / sub-pixel variance size, sse, the open-loop ME
 * and MD full-pel search kernels) and the 8 <-> 16-bit frame conversions (aom_dsp_rtcd.h, common_dsp_rtcd.h) */
static inline void svtgpu_install_me_md_rtcd(void) {
    svt_aom_highbd_10_variance128x128         = svtgpu_aom_highbd_10_variance128x128;
    svt_aom_highbd_10_variance128x64          = svtgpu_aom_highbd_10_variance128x64;
    svt_aom_highbd_10_variance16x16           = svtgpu_aom_highbd_10_variance16x16;
    svt_aom_highbd_10_variance16x32           = svtgpu_aom_highbd_10_variance16x32;
    svt_aom_highbd_10_variance16x4            = svtgpu_aom_highbd_10_variance16x4;
    svt_aom_highbd_10_variance16x64           = svtgpu_aom_highbd_10_variance16x64;
    svt_aom_highbd_10_variance16x8            = svtgpu_aom_highbd_10_variance16x8;
    svt_aom_highbd_10_variance32x16           = svtgpu_aom_highbd_10_variance32x16;
    svt_aom_highbd_10_variance32x32           = svtgpu_aom_highbd_10_variance32x32;
    svt_aom_highbd_10_variance32x64           = svtgpu_aom_highbd_10_variance32x64;
    svt_aom_highbd_10_variance32x8            = svtgpu_aom_highbd_10_variance32x8;
    svt_aom_highbd_10_variance4x16            = svtgpu_aom_highbd_10_variance4x16;
    svt_aom_highbd_10_variance4x4             = svtgpu_aom_highbd_10_variance4x4;
    svt_aom_highbd_10_variance4x8             = svtgpu_aom_highbd_10_variance4x8;
    svt_aom_highbd_10_variance64x128          = svtgpu_aom_highbd_10_variance64x128;
    svt_aom_highbd_10_variance64x16           = svtgpu_aom_highbd_10_variance64x16;
    svt_aom_highbd_10_variance64x32           = svtgpu_aom_highbd_10_variance64x32;
    svt_aom_highbd_10_variance64x64           = svtgpu_aom_highbd_10_variance64x64;
    svt_aom_highbd_10_variance8x16            = svtgpu_aom_highbd_10_variance8x16;
    svt_aom_highbd_10_variance8x32            = svtgpu_aom_highbd_10_variance8x32;
    svt_aom_highbd_10_variance8x4             = svtgpu_aom_highbd_10_variance8x4;
    svt_aom_highbd_10_variance8x8             = svtgpu_aom_highbd_10_variance8x8;
    svt_aom_highbd_sse                        = svtgpu_aom_highbd_sse;
    svt_aom_sad128x128                        = svtgpu_aom_sad128x128;
    svt_aom_sad128x128x4d                     = svtgpu_aom_sad128x128x4d;
    svt_aom_sad128x64                         = svtgpu_aom_sad128x64;
    svt_aom_sad128x64x4d                      = svtgpu_aom_sad128x64x4d;
    svt_aom_sad16x16                          = svtgpu_aom_sad16x16;
    svt_aom_sad16x16x4d                       = svtgpu_aom_sad16x16x4d;
    svt_aom_sad16x32                          = svtgpu_aom_sad16x32;
    svt_aom_sad16x32x4d                       = svtgpu_aom_sad16x32x4d;
    svt_aom_sad16x4                           = svtgpu_aom_sad16x4;
    svt_aom_sad16x4x4d                        = svtgpu_aom_sad16x4x4d;
    svt_aom_sad16x64                          = svtgpu_aom_sad16x64;
    svt_aom_sad16x64x4d                       = svtgpu_aom_sad16x64x4d;
    svt_aom_sad16x8                           = svtgpu_aom_sad16x8;
    svt_aom_sad16x8x4d                        = svtgpu_aom_sad16x8x4d;
    svt_aom_sad32x16                          = svtgpu_aom_sad32x16;
    svt_aom_sad32x16x4d                       = svtgpu_aom_sad32x16x4d;
    svt_aom_sad32x32                          = svtgpu_aom_sad32x32;
    svt_aom_sad32x32x4d                       = svtgpu_aom_sad32x32x4d;
    svt_aom_sad32x64                          = svtgpu_aom_sad32x64;
    svt_aom_sad32x64x4d                       = svtgpu_aom_sad32x64x4d;
    svt_aom_sad32x8                           = svtgpu_aom_sad32x8;
    svt_aom_sad32x8x4d                        = svtgpu_aom_sad32x8x4d;
    svt_aom_sad4x16                           = svtgpu_aom_sad4x16;
    svt_aom_sad4x16x4d                        = svtgpu_aom_sad4x16x4d;
    svt_aom_sad4x4                            = svtgpu_aom_sad4x4;
    svt_aom_sad4x4x4d                         = svtgpu_aom_sad4x4x4d;
    svt_aom_sad4x8                            = svtgpu_aom_sad4x8;
    svt_aom_sad4x8x4d                         = svtgpu_aom_sad4x8x4d;
    svt_aom_sad64x128                         = svtgpu_aom_sad64x128;
    svt_aom_sad64x128x4d                      = svtgpu_aom_sad64x128x4d;
    svt_aom_sad64x16                          = svtgpu_aom_sad64x16;
    svt_aom_sad64x16x4d                       = svtgpu_aom_sad64x16x4d;
    svt_aom_sad64x32                          = svtgpu_aom_sad64x32;
    svt_aom_sad64x32x4d                       = svtgpu_aom_sad64x32x4d;
    svt_aom_sad64x64                          = svtgpu_aom_sad64x64;
    svt_aom_sad64x64x4d                       = svtgpu_aom_sad64x64x4d;
    svt_aom_sad8x16                           = svtgpu_aom_sad8x16;
    svt_aom_sad8x16x4d                        = svtgpu_aom_sad8x16x4d;
    svt_aom_sad8x32                           = svtgpu_aom_sad8x32;
    svt_aom_sad8x32x4d                        = svtgpu_aom_sad8x32x4d;
    svt_aom_sad8x4                            = svtgpu_aom_sad8x4;
    svt_aom_sad8x4x4d                         = svtgpu_aom_sad8x4x4d;
    svt_aom_sad8x8                            = svtgpu_aom_sad8x8;
    svt_aom_sad8x8x4d                         = svtgpu_aom_sad8x8x4d;
    svt_aom_sse                               = svtgpu_aom_sse;
    svt_aom_sub_pixel_variance128x128         = svtgpu_aom_sub_pixel_variance128x128;
    svt_aom_sub_pixel_variance128x64          = svtgpu_aom_sub_pixel_variance128x64;
    svt_aom_sub_pixel_variance16x16           = svtgpu_aom_sub_pixel_variance16x16;
    svt_aom_sub_pixel_variance16x32           = svtgpu_aom_sub_pixel_variance16x32;
    svt_aom_sub_pixel_variance16x4            = svtgpu_aom_sub_pixel_variance16x4;
    svt_aom_sub_pixel_variance16x64           = svtgpu_aom_sub_pixel_variance16x64;
    svt_aom_sub_pixel_variance16x8            = svtgpu_aom_sub_pixel_variance16x8;
    svt_aom_sub_pixel_variance32x16           = svtgpu_aom_sub_pixel_variance32x16;
    svt_aom_sub_pixel_variance32x32           = svtgpu_aom_sub_pixel_variance32x32;
    svt_aom_sub_pixel_variance32x64           = svtgpu_aom_sub_pixel_variance32x64;
    svt_aom_sub_pixel_variance32x8            = svtgpu_aom_sub_pixel_variance32x8;
    svt_aom_sub_pixel_variance4x16            = svtgpu_aom_sub_pixel_variance4x16;
    svt_aom_sub_pixel_variance4x4             = svtgpu_aom_sub_pixel_variance4x4;
    svt_aom_sub_pixel_variance4x8             = svtgpu_aom_sub_pixel_variance4x8;
    svt_aom_sub_pixel_variance64x128          = svtgpu_aom_sub_pixel_variance64x128;
    svt_aom_sub_pixel_variance64x16           = svtgpu_aom_sub_pixel_variance64x16;
    svt_aom_sub_pixel_variance64x32           = svtgpu_aom_sub_pixel_variance64x32;
    svt_aom_sub_pixel_variance64x64           = svtgpu_aom_sub_pixel_variance64x64;
    svt_aom_sub_pixel_variance8x16            = svtgpu_aom_sub_pixel_variance8x16;
    svt_aom_sub_pixel_variance8x32            = svtgpu_aom_sub_pixel_variance8x32;
    svt_aom_sub_pixel_variance8x4             = svtgpu_aom_sub_pixel_variance8x4;
    svt_aom_sub_pixel_variance8x8             = svtgpu_aom_sub_pixel_variance8x8;
    svt_aom_variance128x128                   = svtgpu_aom_variance128x128;
    svt_aom_variance128x64                    = svtgpu_aom_variance128x64;
    svt_aom_variance16x16                     = svtgpu_aom_variance16x16;
    svt_aom_variance16x32                     = svtgpu_aom_variance16x32;
    svt_aom_variance16x4                      = svtgpu_aom_variance16x4;
    svt_aom_variance16x64                     = svtgpu_aom_variance16x64;
    svt_aom_variance16x8                      = svtgpu_aom_variance16x8;
    svt_aom_variance32x16                     = svtgpu_aom_variance32x16;
    svt_aom_variance32x32                     = svtgpu_aom_variance32x32;
    svt_aom_variance32x64                     = svtgpu_aom_variance32x64;
    svt_aom_variance32x8                      = svtgpu_aom_variance32x8;
    svt_aom_variance4x16                      = svtgpu_aom_variance4x16;
    svt_aom_variance4x4                       = svtgpu_aom_variance4x4;
    svt_aom_variance4x8                       = svtgpu_aom_variance4x8;
    svt_aom_variance64x128                    = svtgpu_aom_variance64x128;
    svt_aom_variance64x16                     = svtgpu_aom_variance64x16;
    svt_aom_variance64x32                     = svtgpu_aom_variance64x32;
    svt_aom_variance64x64                     = svtgpu_aom_variance64x64;
    svt_aom_variance8x16                      = svtgpu_aom_variance8x16;
    svt_aom_variance8x32                      = svtgpu_aom_variance8x32;
    svt_aom_variance8x4                       = svtgpu_aom_variance8x4;
    svt_aom_variance8x8                       = svtgpu_aom_variance8x8;
    svt_convert_16bit_to_8bit                 = svtgpu_convert_16bit_to_8bit;
    svt_convert_8bit_to_16bit                 = svtgpu_convert_8bit_to_16bit;
    svt_ext_all_sad_calculation_8x8_16x16     = svtgpu_ext_all_sad_calculation_8x8_16x16;
    svt_ext_eight_sad_calculation_32x32_64x64 = svtgpu_ext_eight_sad_calculation_32x32_64x64;
    svt_ext_sad_calculation_32x32_64x64       = svtgpu_ext_sad_calculation_32x32_64x64;
    svt_ext_sad_calculation_8x8_16x16         = svtgpu_ext_sad_calculation_8x8_16x16;
    svt_nxm_sad_kernel                        = svtgpu_nxm_sad_kernel;
    svt_nxm_sad_kernel_sub_sampled            = svtgpu_nxm_sad_kernel_sub_sampled;
    svt_pme_sad_loop_kernel                   = svtgpu_pme_sad_loop_kernel;
    sad_16b_kernel                            = svtgpu_sad_16b_kernel;
    svt_sad_loop_kernel                       = svtgpu_sad_loop_kernel;
}

/* the OBMC distortion family (aom_dsp_rtcd.h:354-484): obmc sad / variance / sub-pixel variance of the 22 block sizes.
 * init_fn_ptr copies them into svt_aom_mefn_ptr[].osdf / ovf / osvf (av1me.c:171-196), so the install point is the
 * same as for svtgpu_install_me_md_rtcd: before init_fn_ptr (tests/test_obmc.py checks both orders).  Kept apart from
 * that function: an encoder opts into the OBMC shims on their own. */
#define SVTGPU_OBMC_INSTALL(W, H)                                                          \
    svt_aom_obmc_sad##W##x##H                = svtgpu_aom_obmc_sad##W##x##H;                \
    svt_aom_obmc_variance##W##x##H           = svtgpu_aom_obmc_variance##W##x##H;           \
    svt_aom_obmc_sub_pixel_variance##W##x##H = svtgpu_aom_obmc_sub_pixel_variance##W##x##H;
static inline void svtgpu_install_obmc_rtcd(void) {
    SVTGPU_OBMC_INSTALL(4, 4)
    SVTGPU_OBMC_INSTALL(4, 8)
    SVTGPU_OBMC_INSTALL(8, 4)
    SVTGPU_OBMC_INSTALL(8, 8)
    SVTGPU_OBMC_INSTALL(8, 16)
    SVTGPU_OBMC_INSTALL(16, 8)
    SVTGPU_OBMC_INSTALL(16, 16)
    SVTGPU_OBMC_INSTALL(16, 32)
    SVTGPU_OBMC_INSTALL(32, 16)
    SVTGPU_OBMC_INSTALL(32, 32)
    SVTGPU_OBMC_INSTALL(32, 64)
    SVTGPU_OBMC_INSTALL(64, 32)
    SVTGPU_OBMC_INSTALL(64, 64)
    SVTGPU_OBMC_INSTALL(64, 128)
    SVTGPU_OBMC_INSTALL(128, 64)
    SVTGPU_OBMC_INSTALL(128, 128)
    SVTGPU_OBMC_INSTALL(4, 16)
    SVTGPU_OBMC_INSTALL(16, 4)
    SVTGPU_OBMC_INSTALL(8, 32)
    SVTGPU_OBMC_INSTALL(32, 8)
    SVTGPU_OBMC_INSTALL(16, 64)
    SVTGPU_OBMC_INSTALL(64, 16)
}
#undef SVTGPU_OBMC_INSTALL

/* the non-normative frame resizer's two plane functions (aom_dsp_rtcd.h:898-901), which svt_aom_resize_frame calls per
 * plane (EbResize.c:889-935); nothing copies these pointers, so any point after the RTCD setup will do.  An encoder that
 * keeps its pictures on the device calls svtgpu_resize_frame instead. */
static inline void svtgpu_install_resize_rtcd(void) {
    svt_av1_resize_plane        = svtgpu_av1_resize_plane;
    svt_av1_highbd_resize_plane = svtgpu_av1_highbd_resize_plane;
}

/* The temporal filter's filter half (aom_dsp_rtcd.h:795-835, 874-877): nine pointers.  The two noise estimates are plain C
 * and the library exports them.  The other seven take struct MeContext * (and EbPictureBufferDesc *), whose layouts the
 * library does not know, so the adapters below -- compiled here, inside the encoder, where those types are complete --
 * read the fields (tf_block_row / tf_block_col, the split flags, motion vectors and block errors, tf_decay_factor_fp16,
 * tf_mv_dist_th, tf_chroma; stride_y of the picture) and call the library's plain-C shims.  Opt-in: define
 * SVTGPU_RTCD_WITH_TF before including this header, in a unit that has included EbMotionEstimationContext.h and
 * EbPictureBufferDesc.h.  Nothing copies these pointers, so any point after the RTCD setup will do.  An encoder that keeps
 * its pictures on the device calls svtgpu_tf_filter_frame instead. */
#ifdef SVTGPU_RTCD_WITH_TF
static void svtgpu_tf_read_me_context(const struct MeContext *c, SvtGpuTfBlock *b, SvtGpuTfParams *p) {
    for (int i = 0; i < 4; i++) {
        b->split32[i] = c->tf_32x32_block_split_flag[i];
        b->mv32_x[i] = c->tf_32x32_mv_x[i], b->mv32_y[i] = c->tf_32x32_mv_y[i];
        b->err32[i] = c->tf_32x32_block_error[i];
    }
    for (int i = 0; i < 16; i++) {
        b->mv16_x[i] = c->tf_16x16_mv_x[i], b->mv16_y[i] = c->tf_16x16_mv_y[i];
        b->err16[i] = c->tf_16x16_block_error[i];
    }
    for (int i = 0; i < 3; i++) p->decay_factor_fp16[i] = c->tf_decay_factor_fp16[i];
    p->mv_dist_th = c->tf_mv_dist_th, p->tf_chroma = c->tf_chroma;
    p->bit_depth = 0, p->use_zz_based_filter = 0; /* named by the entry that is called */
}
static void svtgpu_adapt_tf_planewise_medium(struct MeContext *me_ctx, const uint8_t *y_src, int y_src_stride,
                                             const uint8_t *y_pre, int y_pre_stride, const uint8_t *u_src,
                                             const uint8_t *v_src, int uv_src_stride, const uint8_t *u_pre,
                                             const uint8_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                             unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum,
                                             uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum,
                                             uint16_t *v_count) {
    SvtGpuTfBlock  b;
    SvtGpuTfParams p;
    svtgpu_tf_read_me_context(me_ctx, &b, &p);
    svtgpu_tf_apply_planewise_medium(&b, me_ctx->tf_block_col + me_ctx->tf_block_row * 2, &p, y_src, y_src_stride, y_pre,
                                     y_pre_stride, u_src, v_src, uv_src_stride, u_pre, v_pre, uv_pre_stride, block_width,
                                     block_height, ss_x, ss_y, y_accum, y_count, u_accum, u_count, v_accum, v_count);
}
static void svtgpu_adapt_tf_planewise_medium_hbd(struct MeContext *me_ctx, const uint16_t *y_src, int y_src_stride,
                                                 const uint16_t *y_pre, int y_pre_stride, const uint16_t *u_src,
                                                 const uint16_t *v_src, int uv_src_stride, const uint16_t *u_pre,
                                                 const uint16_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                                 unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum,
                                                 uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                                 uint32_t *v_accum, uint16_t *v_count, uint32_t encoder_bit_depth) {
    SvtGpuTfBlock  b;
    SvtGpuTfParams p;
    svtgpu_tf_read_me_context(me_ctx, &b, &p);
    svtgpu_tf_apply_planewise_medium_hbd(&b, me_ctx->tf_block_col + me_ctx->tf_block_row * 2, &p, y_src, y_src_stride,
                                         y_pre, y_pre_stride, u_src, v_src, uv_src_stride, u_pre, v_pre, uv_pre_stride,
                                         block_width, block_height, ss_x, ss_y, y_accum, y_count, u_accum, u_count, v_accum,
                                         v_count, encoder_bit_depth);
}
static void svtgpu_adapt_tf_zz_planewise_medium(struct MeContext *me_ctx, const uint8_t *y_pre, int y_pre_stride,
                                                const uint8_t *u_pre, const uint8_t *v_pre, int uv_pre_stride,
                                                unsigned int block_width, unsigned int block_height, int ss_x, int ss_y,
                                                uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                                uint32_t *v_accum, uint16_t *v_count) {
    SvtGpuTfBlock  b;
    SvtGpuTfParams p;
    svtgpu_tf_read_me_context(me_ctx, &b, &p);
    svtgpu_tf_apply_zz_planewise_medium(&b, me_ctx->tf_block_col + me_ctx->tf_block_row * 2, &p, y_pre, y_pre_stride, u_pre,
                                        v_pre, uv_pre_stride, block_width, block_height, ss_x, ss_y, y_accum, y_count,
                                        u_accum, u_count, v_accum, v_count);
}
static void svtgpu_adapt_tf_zz_planewise_medium_hbd(struct MeContext *me_ctx, const uint16_t *y_pre, int y_pre_stride,
                                                    const uint16_t *u_pre, const uint16_t *v_pre, int uv_pre_stride,
                                                    unsigned int block_width, unsigned int block_height, int ss_x,
                                                    int ss_y, uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum,
                                                    uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count,
                                                    uint32_t encoder_bit_depth) {
    SvtGpuTfBlock  b;
    SvtGpuTfParams p;
    svtgpu_tf_read_me_context(me_ctx, &b, &p);
    svtgpu_tf_apply_zz_planewise_medium_hbd(&b, me_ctx->tf_block_col + me_ctx->tf_block_row * 2, &p, y_pre, y_pre_stride,
                                            u_pre, v_pre, uv_pre_stride, block_width, block_height, ss_x, ss_y, y_accum,
                                            y_count, u_accum, u_count, v_accum, v_count, encoder_bit_depth);
}
static void svtgpu_adapt_tf_get_final_filtered_pixels(struct MeContext *me_ctx, EbByte *src_center_ptr_start,
                                                      uint16_t **altref_buffer_highbd_start, uint32_t **accum,
                                                      uint16_t **count, const uint32_t *stride, int blk_y_src_offset,
                                                      int blk_ch_src_offset, uint16_t blk_width_ch, uint16_t blk_height_ch,
                                                      Bool is_highbd) {
    svtgpu_tf_get_final_filtered_pixels(me_ctx->tf_chroma, src_center_ptr_start, altref_buffer_highbd_start, accum, count,
                                        stride, blk_y_src_offset, blk_ch_src_offset, blk_width_ch, blk_height_ch,
                                        is_highbd ? 1 : 0);
}
static void svtgpu_adapt_tf_filtering_central(struct MeContext *me_ctx, EbPictureBufferDesc *input_picture_ptr_central,
                                              EbByte *src, uint32_t **accum, uint16_t **count, uint16_t blk_width,
                                              uint16_t blk_height, uint32_t ss_x, uint32_t ss_y) {
    svtgpu_tf_apply_filtering_central(me_ctx->tf_chroma, input_picture_ptr_central->stride_y, src, accum, count, blk_width,
                                      blk_height, ss_x, ss_y);
}
static void svtgpu_adapt_tf_filtering_central_highbd(struct MeContext *me_ctx,
                                                     EbPictureBufferDesc *input_picture_ptr_central, uint16_t **src_16bit,
                                                     uint32_t **accum, uint16_t **count, uint16_t blk_width,
                                                     uint16_t blk_height, uint32_t ss_x, uint32_t ss_y) {
    svtgpu_tf_apply_filtering_central_highbd(me_ctx->tf_chroma, input_picture_ptr_central->stride_y, src_16bit, accum,
                                             count, blk_width, blk_height, ss_x, ss_y);
}
static inline void svtgpu_install_tf_rtcd(void) {
    svt_av1_apply_temporal_filter_planewise_medium              = svtgpu_adapt_tf_planewise_medium;
    svt_av1_apply_temporal_filter_planewise_medium_hbd          = svtgpu_adapt_tf_planewise_medium_hbd;
    svt_av1_apply_zz_based_temporal_filter_planewise_medium     = svtgpu_adapt_tf_zz_planewise_medium;
    svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd = svtgpu_adapt_tf_zz_planewise_medium_hbd;
    get_final_filtered_pixels                                   = svtgpu_adapt_tf_get_final_filtered_pixels;
    apply_filtering_central                                     = svtgpu_adapt_tf_filtering_central;
    apply_filtering_central_highbd                              = svtgpu_adapt_tf_filtering_central_highbd;
    svt_estimate_noise_fp16                                     = svtgpu_estimate_noise_fp16;
    svt_estimate_noise_highbd_fp16                              = svtgpu_estimate_noise_highbd_fp16;
}
/* 1 when pointer k (0..8, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_tf_rtcd_installed(int k) {
    switch (k) {
    case 0: return svt_av1_apply_temporal_filter_planewise_medium == svtgpu_adapt_tf_planewise_medium;
    case 1: return svt_av1_apply_temporal_filter_planewise_medium_hbd == svtgpu_adapt_tf_planewise_medium_hbd;
    case 2: return svt_av1_apply_zz_based_temporal_filter_planewise_medium == svtgpu_adapt_tf_zz_planewise_medium;
    case 3: return svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd == svtgpu_adapt_tf_zz_planewise_medium_hbd;
    case 4: return get_final_filtered_pixels == svtgpu_adapt_tf_get_final_filtered_pixels;
    case 5: return apply_filtering_central == svtgpu_adapt_tf_filtering_central;
    case 6: return apply_filtering_central_highbd == svtgpu_adapt_tf_filtering_central_highbd;
    case 7: return svt_estimate_noise_fp16 == svtgpu_estimate_noise_fp16;
    case 8: return svt_estimate_noise_highbd_fp16 == svtgpu_estimate_noise_highbd_fp16;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_TF */

/* The single-reference interpolation family (common_dsp_rtcd.h: svt_av1_convolve_{2d,x,y,2d_copy}_sr and the four
 * svt_av1_highbd_convolve_*_sr): eight pointers.  They take the reference's InterpFilterParams / ConvolveParams, whose
 * layouts the library does not know, so the adapters below -- compiled here, where those types are complete (convolve.h)
 * -- pick the kernel row of the phase with av1_get_interp_filter_subpel_kernel, read round_0 / round_1 and call the
 * library's plain-C shims.  Opt-in: define SVTGPU_RTCD_WITH_INTERP before including this header, in a unit that has
 * included convolve.h.  Install point: after the RTCD setup (EbEncHandle.c:1531) and BEFORE
 * svt_aom_asm_set_convolve_asm_table() (:1533) and svt_aom_asm_set_convolve_hbd_asm_table() (:1537): those two functions
 * COPY the pointers into the svt_aom_convolve[][][] / svt_aom_convolveHbd[][][] tables that svt_inter_predictor and
 * svt_highbd_inter_predictor call, so an install after them changes nothing the encoder calls. */
#ifdef SVTGPU_RTCD_WITH_INTERP
#define SVTGPU_ADAPT_CONVOLVE(name)                                                                                        \
    static void svtgpu_adapt_convolve_##name(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride,     \
                                             int32_t w, int32_t h, InterpFilterParams *filter_params_x,                    \
                                             InterpFilterParams *filter_params_y, const int32_t subpel_x_q4,               \
                                             const int32_t subpel_y_q4, ConvolveParams *conv_params) {                     \
        svtgpu_av1_convolve_##name(                                                                                        \
            src, src_stride, dst, dst_stride, w, h,                                                                        \
            filter_params_x ? av1_get_interp_filter_subpel_kernel(*filter_params_x, subpel_x_q4 & SUBPEL_MASK) : NULL,     \
            filter_params_y ? av1_get_interp_filter_subpel_kernel(*filter_params_y, subpel_y_q4 & SUBPEL_MASK) : NULL,     \
            conv_params->round_0, conv_params->round_1);                                                                   \
    }                                                                                                                      \
    static void svtgpu_adapt_highbd_convolve_##name(const uint16_t *src, int32_t src_stride, uint16_t *dst,                \
                                                    int32_t dst_stride, int32_t w, int32_t h,                              \
                                                    const InterpFilterParams *filter_params_x,                             \
                                                    const InterpFilterParams *filter_params_y, const int32_t subpel_x_q4,  \
                                                    const int32_t subpel_y_q4, ConvolveParams *conv_params, int32_t bd) {  \
        svtgpu_av1_highbd_convolve_##name(                                                                                 \
            src, src_stride, dst, dst_stride, w, h,                                                                        \
            filter_params_x ? av1_get_interp_filter_subpel_kernel(*filter_params_x, subpel_x_q4 & SUBPEL_MASK) : NULL,     \
            filter_params_y ? av1_get_interp_filter_subpel_kernel(*filter_params_y, subpel_y_q4 & SUBPEL_MASK) : NULL,     \
            conv_params->round_0, conv_params->round_1, bd);                                                               \
    }
SVTGPU_ADAPT_CONVOLVE(2d_sr)
SVTGPU_ADAPT_CONVOLVE(x_sr)
SVTGPU_ADAPT_CONVOLVE(y_sr)
SVTGPU_ADAPT_CONVOLVE(2d_copy_sr)
#undef SVTGPU_ADAPT_CONVOLVE
static inline void svtgpu_install_interp_rtcd(void) {
    svt_av1_convolve_2d_sr             = svtgpu_adapt_convolve_2d_sr;
    svt_av1_convolve_x_sr              = svtgpu_adapt_convolve_x_sr;
    svt_av1_convolve_y_sr              = svtgpu_adapt_convolve_y_sr;
    svt_av1_convolve_2d_copy_sr        = svtgpu_adapt_convolve_2d_copy_sr;
    svt_av1_highbd_convolve_2d_sr      = svtgpu_adapt_highbd_convolve_2d_sr;
    svt_av1_highbd_convolve_x_sr       = svtgpu_adapt_highbd_convolve_x_sr;
    svt_av1_highbd_convolve_y_sr       = svtgpu_adapt_highbd_convolve_y_sr;
    svt_av1_highbd_convolve_2d_copy_sr = svtgpu_adapt_highbd_convolve_2d_copy_sr;
}
/* 1 when pointer k (0..7, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_interp_rtcd_installed(int k) {
    switch (k) {
    case 0: return svt_av1_convolve_2d_sr == svtgpu_adapt_convolve_2d_sr;
    case 1: return svt_av1_convolve_x_sr == svtgpu_adapt_convolve_x_sr;
    case 2: return svt_av1_convolve_y_sr == svtgpu_adapt_convolve_y_sr;
    case 3: return svt_av1_convolve_2d_copy_sr == svtgpu_adapt_convolve_2d_copy_sr;
    case 4: return svt_av1_highbd_convolve_2d_sr == svtgpu_adapt_highbd_convolve_2d_sr;
    case 5: return svt_av1_highbd_convolve_x_sr == svtgpu_adapt_highbd_convolve_x_sr;
    case 6: return svt_av1_highbd_convolve_y_sr == svtgpu_adapt_highbd_convolve_y_sr;
    case 7: return svt_av1_highbd_convolve_2d_copy_sr == svtgpu_adapt_highbd_convolve_2d_copy_sr;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_INTERP */

/* The compound (two-reference) family (common_dsp_rtcd.h: svt_av1_jnt_convolve_{2d,x,y,2d_copy} and the four
 * svt_av1_highbd_jnt_convolve_*): eight pointers, the [][][1] half of svt_aom_convolve / svt_aom_convolveHbd.  The adapters
 * pick the kernel rows as the single-reference ones do and spell the ConvolveParams out: round_0, round_1, dst,
 * dst_stride, do_average, use_jnt_comp_avg, fwd_offset, bck_offset.  Opt-in: define SVTGPU_RTCD_WITH_COMPOUND before
 * including this header, in a unit that has included convolve.h.  The install point is svtgpu_install_interp_rtcd's:
 * after the RTCD setup and BEFORE svt_aom_asm_set_convolve_asm_table() / svt_aom_asm_set_convolve_hbd_asm_table(), which
 * copy the pointers. */
#ifdef SVTGPU_RTCD_WITH_COMPOUND
#define SVTGPU_ADAPT_JNT_CONVOLVE(name)                                                                                    \
    static void svtgpu_adapt_jnt_convolve_##name(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, \
                                                 int32_t w, int32_t h, InterpFilterParams *filter_params_x,                \
                                                 InterpFilterParams *filter_params_y, const int32_t subpel_x_q4,           \
                                                 const int32_t subpel_y_q4, ConvolveParams *conv_params) {                 \
        svtgpu_av1_jnt_convolve_##name(                                                                                    \
            src, src_stride, dst, dst_stride, w, h,                                                                        \
            filter_params_x ? av1_get_interp_filter_subpel_kernel(*filter_params_x, subpel_x_q4 & SUBPEL_MASK) : NULL,     \
            filter_params_y ? av1_get_interp_filter_subpel_kernel(*filter_params_y, subpel_y_q4 & SUBPEL_MASK) : NULL,     \
            conv_params->round_0, conv_params->round_1, conv_params->dst, conv_params->dst_stride, conv_params->do_average, \
            conv_params->use_jnt_comp_avg, conv_params->fwd_offset, conv_params->bck_offset);                              \
    }                                                                                                                      \
    static void svtgpu_adapt_highbd_jnt_convolve_##name(                                                                   \
        const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride, int32_t w, int32_t h,                  \
        const InterpFilterParams *filter_params_x, const InterpFilterParams *filter_params_y, const int32_t subpel_x_q4,   \
        const int32_t subpel_y_q4, ConvolveParams *conv_params, int32_t bd) {                                              \
        svtgpu_av1_highbd_jnt_convolve_##name(                                                                             \
            src, src_stride, dst, dst_stride, w, h,                                                                        \
            filter_params_x ? av1_get_interp_filter_subpel_kernel(*filter_params_x, subpel_x_q4 & SUBPEL_MASK) : NULL,     \
            filter_params_y ? av1_get_interp_filter_subpel_kernel(*filter_params_y, subpel_y_q4 & SUBPEL_MASK) : NULL,     \
            conv_params->round_0, conv_params->round_1, conv_params->dst, conv_params->dst_stride, conv_params->do_average, \
            conv_params->use_jnt_comp_avg, conv_params->fwd_offset, conv_params->bck_offset, bd);                          \
    }
SVTGPU_ADAPT_JNT_CONVOLVE(2d)
SVTGPU_ADAPT_JNT_CONVOLVE(x)
SVTGPU_ADAPT_JNT_CONVOLVE(y)
SVTGPU_ADAPT_JNT_CONVOLVE(2d_copy)
#undef SVTGPU_ADAPT_JNT_CONVOLVE
static inline void svtgpu_install_compound_rtcd(void) {
    svt_av1_jnt_convolve_2d             = svtgpu_adapt_jnt_convolve_2d;
    svt_av1_jnt_convolve_x              = svtgpu_adapt_jnt_convolve_x;
    svt_av1_jnt_convolve_y              = svtgpu_adapt_jnt_convolve_y;
    svt_av1_jnt_convolve_2d_copy        = svtgpu_adapt_jnt_convolve_2d_copy;
    svt_av1_highbd_jnt_convolve_2d      = svtgpu_adapt_highbd_jnt_convolve_2d;
    svt_av1_highbd_jnt_convolve_x       = svtgpu_adapt_highbd_jnt_convolve_x;
    svt_av1_highbd_jnt_convolve_y       = svtgpu_adapt_highbd_jnt_convolve_y;
    svt_av1_highbd_jnt_convolve_2d_copy = svtgpu_adapt_highbd_jnt_convolve_2d_copy;
}
/* 1 when pointer i (0..7, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_compound_rtcd_bound(int i) {
    switch (i) {
    case 0: return svt_av1_jnt_convolve_2d == svtgpu_adapt_jnt_convolve_2d;
    case 1: return svt_av1_jnt_convolve_x == svtgpu_adapt_jnt_convolve_x;
    case 2: return svt_av1_jnt_convolve_y == svtgpu_adapt_jnt_convolve_y;
    case 3: return svt_av1_jnt_convolve_2d_copy == svtgpu_adapt_jnt_convolve_2d_copy;
    case 4: return svt_av1_highbd_jnt_convolve_2d == svtgpu_adapt_highbd_jnt_convolve_2d;
    case 5: return svt_av1_highbd_jnt_convolve_x == svtgpu_adapt_highbd_jnt_convolve_x;
    case 6: return svt_av1_highbd_jnt_convolve_y == svtgpu_adapt_highbd_jnt_convolve_y;
    case 7: return svt_av1_highbd_jnt_convolve_2d_copy == svtgpu_adapt_highbd_jnt_convolve_2d_copy;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_COMPOUND */
/* The masked compound family (common_dsp_rtcd.h: svt_av1_build_compound_diffwtd_mask_d16, svt_aom_lowbd_blend_a64_d16_mask,
 * svt_aom_highbd_blend_a64_d16_mask): three pointers, what av1_make_masked_scaled_inter_predictor and
 * svt_aom_build_masked_compound_no_round call for COMPOUND_DIFFWTD and COMPOUND_WEDGE.  The adapters spell the
 * ConvolveParams out as round_0, round_1.  Opt-in: define SVTGPU_RTCD_WITH_MASKED_COMPOUND before including this header, in a
 * unit that has included convolve.h.  Install after the RTCD setup; nothing copies these pointers. */
#ifdef SVTGPU_RTCD_WITH_MASKED_COMPOUND
static void svtgpu_adapt_build_compound_diffwtd_mask_d16(uint8_t *mask, DIFFWTD_MASK_TYPE mask_type, const CONV_BUF_TYPE *src0,
                                                         int src0_stride, const CONV_BUF_TYPE *src1, int src1_stride, int h,
                                                         int w, ConvolveParams *conv_params, int bd) {
    svtgpu_av1_build_compound_diffwtd_mask_d16(mask, (int32_t)mask_type, src0, src0_stride, src1, src1_stride, h, w,
                                               conv_params->round_0, conv_params->round_1, bd);
}
static void svtgpu_adapt_lowbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const CONV_BUF_TYPE *src0,
                                                  uint32_t src0_stride, const CONV_BUF_TYPE *src1, uint32_t src1_stride,
                                                  const uint8_t *mask, uint32_t mask_stride, int w, int h, int subw, int subh,
                                                  ConvolveParams *conv_params) {
    svtgpu_aom_lowbd_blend_a64_d16_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subw,
                                        subh, conv_params->round_0, conv_params->round_1);
}
static void svtgpu_adapt_highbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const CONV_BUF_TYPE *src0,
                                                   uint32_t src0_stride, const CONV_BUF_TYPE *src1, uint32_t src1_stride,
                                                   const uint8_t *mask, uint32_t mask_stride, int w, int h, int subx, int suby,
                                                   ConvolveParams *conv_params, const int bd) {
    svtgpu_aom_highbd_blend_a64_d16_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subx,
                                         suby, conv_params->round_0, conv_params->round_1, bd);
}
static inline void svtgpu_install_masked_compound_rtcd(void) {
    svt_av1_build_compound_diffwtd_mask_d16 = svtgpu_adapt_build_compound_diffwtd_mask_d16;
    svt_aom_lowbd_blend_a64_d16_mask        = svtgpu_adapt_lowbd_blend_a64_d16_mask;
    svt_aom_highbd_blend_a64_d16_mask       = svtgpu_adapt_highbd_blend_a64_d16_mask;
}
/* 1 when pointer i (0..2, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_masked_compound_rtcd_bound(int i) {
    switch (i) {
    case 0: return svt_av1_build_compound_diffwtd_mask_d16 == svtgpu_adapt_build_compound_diffwtd_mask_d16;
    case 1: return svt_aom_lowbd_blend_a64_d16_mask == svtgpu_adapt_lowbd_blend_a64_d16_mask;
    case 2: return svt_aom_highbd_blend_a64_d16_mask == svtgpu_adapt_highbd_blend_a64_d16_mask;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_MASKED_COMPOUND */
/* The OBMC blends (common_dsp_rtcd.h: svt_aom_blend_a64_vmask / _hmask, svt_aom_highbd_blend_a64_vmask_16bit / _hmask_16bit,
 * svt_aom_highbd_blend_a64_vmask_8bit / _hmask_8bit): six pointers, what build_obmc_inter_pred_above / _left call per
 * neighbour and plane (the _8bit forms serve the inter-intra smooth masks).  Kept apart from svtgpu_install_obmc_rtcd(), the
 * OBMC distortion family.  Opt-in: define SVTGPU_RTCD_WITH_OBMC_BLEND before including this header.  Install after the RTCD
 * setup; nothing copies these pointers.  An encoder whose reference pictures are on the device does not need them: it calls
 * svtgpu_obmc_predict_batch instead. */
#ifdef SVTGPU_RTCD_WITH_OBMC_BLEND
#define SVTGPU_ADAPT_BLEND8(name)                                                                                              \
    static void svtgpu_adapt_##name(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,              \
                                    const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int w, int h) {            \
        svtgpu_aom_##name(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h);                                  \
    }
#define SVTGPU_ADAPT_BLEND_BD(name, T)                                                                                         \
    static void svtgpu_adapt_##name(T *dst, uint32_t dst_stride, const T *src0, uint32_t src0_stride, const T *src1,           \
                                    uint32_t src1_stride, const uint8_t *mask, int w, int h, int bd) {                         \
        svtgpu_aom_##name(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, w, h, bd);                              \
    }
SVTGPU_ADAPT_BLEND8(blend_a64_vmask)
SVTGPU_ADAPT_BLEND8(blend_a64_hmask)
SVTGPU_ADAPT_BLEND_BD(highbd_blend_a64_vmask_16bit, uint16_t)
SVTGPU_ADAPT_BLEND_BD(highbd_blend_a64_hmask_16bit, uint16_t)
SVTGPU_ADAPT_BLEND_BD(highbd_blend_a64_vmask_8bit, uint8_t)
SVTGPU_ADAPT_BLEND_BD(highbd_blend_a64_hmask_8bit, uint8_t)
static inline void svtgpu_install_obmc_blend_rtcd(void) {
    svt_aom_blend_a64_vmask              = svtgpu_adapt_blend_a64_vmask;
    svt_aom_blend_a64_hmask              = svtgpu_adapt_blend_a64_hmask;
    svt_aom_highbd_blend_a64_vmask_16bit = svtgpu_adapt_highbd_blend_a64_vmask_16bit;
    svt_aom_highbd_blend_a64_hmask_16bit = svtgpu_adapt_highbd_blend_a64_hmask_16bit;
    svt_aom_highbd_blend_a64_vmask_8bit  = svtgpu_adapt_highbd_blend_a64_vmask_8bit;
    svt_aom_highbd_blend_a64_hmask_8bit  = svtgpu_adapt_highbd_blend_a64_hmask_8bit;
}
/* 1 when pointer i (0..5, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_obmc_blend_rtcd_bound(int i) {
    switch (i) {
    case 0: return svt_aom_blend_a64_vmask == svtgpu_adapt_blend_a64_vmask;
    case 1: return svt_aom_blend_a64_hmask == svtgpu_adapt_blend_a64_hmask;
    case 2: return svt_aom_highbd_blend_a64_vmask_16bit == svtgpu_adapt_highbd_blend_a64_vmask_16bit;
    case 3: return svt_aom_highbd_blend_a64_hmask_16bit == svtgpu_adapt_highbd_blend_a64_hmask_16bit;
    case 4: return svt_aom_highbd_blend_a64_vmask_8bit == svtgpu_adapt_highbd_blend_a64_vmask_8bit;
    case 5: return svt_aom_highbd_blend_a64_hmask_8bit == svtgpu_adapt_highbd_blend_a64_hmask_8bit;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_OBMC_BLEND */
/* Warped motion (common_dsp_rtcd.h: svt_av1_warp_affine, svt_av1_highbd_warp_affine): two pointers, what svt_warp_plane /
 * svt_highbd_warp_plane call.  The adapters spell the ConvolveParams out; the shims refuse what the C cannot do (a p_width
 * or p_height that is no multiple of 8, a projection that leaves int32) with a code, which a void pointer cannot carry, so
 * the adapters abort on it.  Opt-in: define SVTGPU_RTCD_WITH_WARP before including this header, in a unit that has included
 * convolve.h.  Install after the RTCD setup; nothing copies these pointers. */
#ifdef SVTGPU_RTCD_WITH_WARP
#include <stdlib.h>
static void svtgpu_adapt_warp_affine(const int32_t *mat, const uint8_t *ref, int width, int height, int stride, uint8_t *pred,
                                     int p_col, int p_row, int p_width, int p_height, int p_stride, int subsampling_x,
                                     int subsampling_y, ConvolveParams *conv_params, int16_t alpha, int16_t beta, int16_t gamma,
                                     int16_t delta) {
    if (svtgpu_av1_warp_affine(mat, ref, width, height, stride, pred, p_col, p_row, p_width, p_height, p_stride, subsampling_x,
                               subsampling_y, conv_params->round_0, conv_params->round_1, conv_params->is_compound,
                               conv_params->dst, conv_params->dst_stride, conv_params->do_average, conv_params->use_jnt_comp_avg,
                               conv_params->fwd_offset, conv_params->bck_offset, alpha, beta, gamma, delta))
        abort();
}
static void svtgpu_adapt_highbd_warp_affine(const int32_t *mat, const uint8_t *ref8b, const uint8_t *ref2b, int width, int height,
                                            int stride8b, int stride2b, uint16_t *pred, int p_col, int p_row, int p_width,
                                            int p_height, int p_stride, int subsampling_x, int subsampling_y, int bd,
                                            ConvolveParams *conv_params, int16_t alpha, int16_t beta, int16_t gamma,
                                            int16_t delta) {
    if (svtgpu_av1_highbd_warp_affine(mat, ref8b, ref2b, width, height, stride8b, stride2b, pred, p_col, p_row, p_width, p_height,
                                      p_stride, subsampling_x, subsampling_y, bd, conv_params->round_0, conv_params->round_1,
                                      conv_params->is_compound, conv_params->dst, conv_params->dst_stride, conv_params->do_average,
                                      conv_params->use_jnt_comp_avg, conv_params->fwd_offset, conv_params->bck_offset, alpha, beta,
                                      gamma, delta))
        abort();
}
static inline void svtgpu_install_warp_rtcd(void) {
    svt_av1_warp_affine        = svtgpu_adapt_warp_affine;
    svt_av1_highbd_warp_affine = svtgpu_adapt_highbd_warp_affine;
}
/* 1 when pointer i (0..1, the order above) is the library's: the adapters are private to the installing unit */
static inline int svtgpu_warp_rtcd_bound(int i) {
    switch (i) {
    case 0: return svt_av1_warp_affine == svtgpu_adapt_warp_affine;
    case 1: return svt_av1_highbd_warp_affine == svtgpu_adapt_highbd_warp_affine;
    default: return 0;
    }
}
#endif /* SVTGPU_RTCD_WITH_WARP */
/* Inter-intra (common_dsp_rtcd.h): the two blends svt_aom_blend_a64_mask / svt_aom_highbd_blend_a64_mask that
 * svt_aom_combine_interintra(_highbd) calls, and the per-size intra predictors svt_aom_(highbd_){dc, dc_top, dc_left, dc_128, v,
 * h, smooth}_predictor_WxH of the ten plane sizes inter-intra reaches: 2 + 2 * 7 * 10 = 142 pointers, each predictor a wrapper
 * of svtgpu_aom_(highbd_)intra_predictor generated from one list.  Opt-in: define SVTGPU_RTCD_WITH_INTERINTRA before including
 * this header.  Install point: after the RTCD setup and BEFORE svt_aom_init_intra_predictors_internal (EbEncHandle.c:1539),
 * which copies the predictor pointers into svt_aom_eb_pred / svt_aom_dc_pred and their highbd tables: build_intra_predictors
 * calls through those tables, so an install after it changes nothing the encoder calls (the interp install's caveat).  The two
 * blend pointers are called directly and may be bound at any time.  An encoder whose reference pictures are on the device
 * does not need them: it calls svtgpu_interintra_predict_batch instead. */
#ifdef SVTGPU_RTCD_WITH_INTERINTRA
#define SVTGPU_II_SIZES(X, k) X(k, 4, 4) X(k, 4, 8) X(k, 8, 4) X(k, 8, 8) X(k, 8, 16) X(k, 16, 8) X(k, 16, 16) X(k, 16, 32) X(k, 32, 16) X(k, 32, 32)
#define SVTGPU_II_KINDS(X)                                                                                                     \
    SVTGPU_II_SIZES(X, dc) SVTGPU_II_SIZES(X, dc_top) SVTGPU_II_SIZES(X, dc_left) SVTGPU_II_SIZES(X, dc_128) SVTGPU_II_SIZES(X, v) \
    SVTGPU_II_SIZES(X, h) SVTGPU_II_SIZES(X, smooth)
enum { svtgpu_ii_kind_dc = SVTGPU_INTRA_DC, svtgpu_ii_kind_dc_top = SVTGPU_INTRA_DC_TOP, svtgpu_ii_kind_dc_left = SVTGPU_INTRA_DC_LEFT,
       svtgpu_ii_kind_dc_128 = SVTGPU_INTRA_DC_128, svtgpu_ii_kind_v = SVTGPU_INTRA_V, svtgpu_ii_kind_h = SVTGPU_INTRA_H,
       svtgpu_ii_kind_smooth = SVTGPU_INTRA_SMOOTH };
#define SVTGPU_II_ADAPT(k, w, h)                                                                                               \
    static void svtgpu_adapt_##k##_predictor_##w##x##h(uint8_t *dst, ptrdiff_t stride, const uint8_t *above, const uint8_t *left) { \
        svtgpu_aom_intra_predictor(dst, stride, above, left, w, h, svtgpu_ii_kind_##k);                                        \
    }                                                                                                                          \
    static void svtgpu_adapt_highbd_##k##_predictor_##w##x##h(uint16_t *dst, ptrdiff_t stride, const uint16_t *above,          \
                                                              const uint16_t *left, int32_t bd) {                              \
        svtgpu_aom_highbd_intra_predictor(dst, stride, above, left, w, h, svtgpu_ii_kind_##k, bd);                             \
    }
SVTGPU_II_KINDS(SVTGPU_II_ADAPT)
static void svtgpu_adapt_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                        const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, uint32_t mask_stride, int w,
                                        int h, int subx, int suby) {
    svtgpu_aom_blend_a64_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subx, suby);
}
static void svtgpu_adapt_highbd_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                               const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, uint32_t mask_stride,
                                               int w, int h, int subx, int suby, int bd) {
    svtgpu_aom_highbd_blend_a64_mask(dst, dst_stride, src0, src0_stride, src1, src1_stride, mask, mask_stride, w, h, subx, suby, bd);
}
#define SVTGPU_II_BIND(k, w, h)                                                                                                \
    svt_aom_##k##_predictor_##w##x##h        = svtgpu_adapt_##k##_predictor_##w##x##h;                                         \
    svt_aom_highbd_##k##_predictor_##w##x##h = svtgpu_adapt_highbd_##k##_predictor_##w##x##h;
static inline void svtgpu_install_interintra_rtcd(void) {
    svt_aom_blend_a64_mask        = svtgpu_adapt_blend_a64_mask;
    svt_aom_highbd_blend_a64_mask = svtgpu_adapt_highbd_blend_a64_mask;
    SVTGPU_II_KINDS(SVTGPU_II_BIND)
}
#define SVTGPU_INTERINTRA_RTCD_COUNT 142
/* 1 when pointer i (0 .. 141) is the library's: 0 and 1 the blends, then per (kind, size) of the list the 8-bit and the highbd
 * pointer; the adapters are private to the installing unit */
#define SVTGPU_II_PROBE(k, w, h)                                                                                               \
    if (i == n++) return svt_aom_##k##_predictor_##w##x##h == svtgpu_adapt_##k##_predictor_##w##x##h;                          \
    if (i == n++) return svt_aom_highbd_##k##_predictor_##w##x##h == svtgpu_adapt_highbd_##k##_predictor_##w##x##h;
static inline int svtgpu_interintra_rtcd_bound(int i) {
    int n = 2;
    if (i == 0) return svt_aom_blend_a64_mask == svtgpu_adapt_blend_a64_mask;
    if (i == 1) return svt_aom_highbd_blend_a64_mask == svtgpu_adapt_highbd_blend_a64_mask;
    SVTGPU_II_KINDS(SVTGPU_II_PROBE)
    return 0;
}
#endif /* SVTGPU_RTCD_WITH_INTERINTRA */
#endif /* SVTGPU_RTCD_H */
