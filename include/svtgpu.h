/*
 * svtgpu.h — C ABI of the MI355X (gfx950) in-loop-filter / distortion library.
 *
 * Drop-in boundary for SVT-AV1 v2.1.0 (reference: GabrielGao0310/SVT-av1_pro-anchor-v2.1.0-).
 * Two layers, both plain C (no HIP or torch types in any signature):
 *
 *  1. RTCD-compatible per-block entry points.  Each has EXACTLY the signature of the reference's
 *     RTCD function pointer it can be assigned to after svt_aom_setup_common_rtcd_internal /
 *     svt_aom_setup_rtcd_internal (Source/Lib/Encoder/Globals/EbEncHandle.c:1530-1531).  They take
 *     host pointers, run the HIP kernel on the library's default device and return the result
 *     synchronously.  They exist for unit parity (the reference's own gtests call these pointers);
 *     they are far too fine-grained to be fast.
 *
 *  2. Frame-level entry points (the real GPU boundary).  They replace the reference's C loops over
 *     64x64 filter blocks (cdef_seg_search, finish_cdef_search, svt_av1_cdef_frame, ...) and run on
 *     device-resident frames.  Every call takes a `void *stream` (a hipStream_t; NULL = the
 *     context's own stream) and is asynchronous with respect to the host unless stated otherwise.
 *
 * Error convention: functions returning int return SVTGPU_OK (0) or a negative SVTGPU_ERR_* code;
 * nothing throws or longjmps across this ABI.  Per-block shims cannot report errors through their
 * reference signature; they abort() with a message if the device is missing (the encoder must not
 * install them without a device — see svtgpu_device_available()).
 */
#ifndef SVTGPU_H
#define SVTGPU_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVTGPU_OK 0
#define SVTGPU_ERR_INVALID_ARG (-1)
#define SVTGPU_ERR_HIP (-2)
#define SVTGPU_ERR_UNSUPPORTED (-3)
#define SVTGPU_ERR_NO_DEVICE (-4)
#define SVTGPU_ERR_OOM (-5)

/* Block-size codes used by the per-block CDEF shims; values equal the reference's BlockSize enum
 * (Source/Lib/Common/Codec/EbDefinitions.h:769-772). */
#define SVTGPU_BLOCK_4X4 0
#define SVTGPU_BLOCK_4X8 1
#define SVTGPU_BLOCK_8X4 2
#define SVTGPU_BLOCK_8X8 3

/* Layout-identical to the reference's CdefList (EbDefinitions.h:253-256). */
typedef struct SvtGpuCdefList {
    uint8_t by;
    uint8_t bx;
} SvtGpuCdefList;

/* Layout-identical to the reference's SgrParamsType (EbDefinitions.h:1768-1771): radii and s values of an ep. */
typedef struct SvtGpuSgrParams {
    int32_t r[2];
    int32_t s[2];
} SvtGpuSgrParams;

/* Layout-identical to the reference's ConvolveParams (EbDefinitions.h:577-590); the Wiener shims read
 * round_0 / round_1 only. */
typedef struct SvtGpuConvolveParams {
    int32_t  ref;
    int32_t  do_average;
    void    *dst;
    int32_t  dst_stride;
    int32_t  round_0;
    int32_t  round_1;
    int32_t  plane;
    int32_t  is_compound;
    int32_t  use_jnt_comp_avg;
    int32_t  fwd_offset;
    int32_t  bck_offset;
    int32_t  use_dist_wtd_comp_avg;
} SvtGpuConvolveParams;

/* Type hooks for a C translation unit compiled against the reference's own headers (INTEGRATION.md §2;
 * oracle/ref_harness/rtcd_bind.c): defining these to CdefList, BlockSize, SgrParamsType, ConvolveParams and
 * EbBitDepth before including this header makes the shim prototypes name the reference's types, so every shim
 * assigns to its RTCD function pointer without a cast.  The layouts are identical, so the ABI is the same. */
#ifndef SVTGPU_CDEF_LIST_T
#define SVTGPU_CDEF_LIST_T SvtGpuCdefList
#endif
#ifndef SVTGPU_BLOCK_SIZE_T
#define SVTGPU_BLOCK_SIZE_T int32_t
#endif
#ifndef SVTGPU_SGR_PARAMS_T
#define SVTGPU_SGR_PARAMS_T SvtGpuSgrParams
#endif
#ifndef SVTGPU_CONVOLVE_PARAMS_T
#define SVTGPU_CONVOLVE_PARAMS_T SvtGpuConvolveParams
#endif
#ifndef SVTGPU_BIT_DEPTH_T
#define SVTGPU_BIT_DEPTH_T int32_t
#endif
/* the return type of the resize shims: EbErrorType in a unit compiled against the reference (svtgpu_rtcd.h); the same
 * 32 bits, 0 = EB_ErrorNone */
#ifndef SVTGPU_ERROR_T
#define SVTGPU_ERROR_T uint32_t
#endif

/* ---------------------------------------------------------------------------------------------
 * Library / device
 * ------------------------------------------------------------------------------------------- */
/* 1 when a gfx950 device is visible and the kernels are loadable, else 0. Never aborts. */
int         svtgpu_device_available(void);
const char *svtgpu_version(void);
/* ABI revision of this header: bumped whenever a struct passed across the boundary changes layout or an entry
 * point changes meaning (6: SvtGpuLrProfile::ms_events, svtgpu_comm_create_bounded, the asynchronous LR search
 * svtgpu_lr_search_frame_async; 7: svtgpu_cdef_apply_frame accepts params == NULL, svtgpu_stream_create; 8: the CCSO entry points,
 * SvtGpuCcsoParams; 9: the OBMC shims and svtgpu_obmc_*; 10: the super-resolution upscale svtgpu_superres_*;
 * 11: the non-normative frame resizer svtgpu_resize_* and its two RTCD shims; 12: the temporal filter's filter half
 * svtgpu_tf_*, SvtGpuTfBlock / SvtGpuTfParams / SvtGpuTfPlanes, and its nine RTCD shims; 13: the eight single-reference
 * interpolation shims svtgpu_av1_(highbd_)convolve_*_sr, SvtGpuTfMotion and svtgpu_tf_predict_frame; 14: the temporal
 * filter's sub-pel search svtgpu_tf_search_frame / _read, SvtGpuTfFullpel / SvtGpuTfSearchParams, and the device chain
 * svtgpu_tf_compensate_filter_frame); 15: the diagnostic read-back svtgpu_lr_read_sgr_planes; 16: the eight compound
 * shims svtgpu_av1_(highbd_)jnt_convolve_*, svtgpu_dist_wtd_weights, SvtGpuCompoundBlock and svtgpu_compound_predict_batch; 17: the masked compounds: the three shims
 * svtgpu_av1_build_compound_diffwtd_mask_d16 / svtgpu_aom_(lowbd|highbd)_blend_a64_d16_mask, svtgpu_wedge_mask,
 * SvtGpuMaskedCompoundBlock and svtgpu_masked_compound_predict_batch; 18: warped motion: the two shims
 * svtgpu_av1_warp_affine / svtgpu_av1_highbd_warp_affine, svtgpu_warp_shear_params, svtgpu_warp_filter_table, SvtGpuWarpBlock
 * and svtgpu_warp_predict_batch; 19: OBMC prediction: svtgpu_obmc_mask, SvtGpuObmcNeighbour / SvtGpuObmcBlock and
 * svtgpu_obmc_predict_batch, the six svtgpu_aom_(highbd_)blend_a64_{v,h}mask shims,
 * svtgpu_obmc_weighted_src_batch and svtgpu_obmc_set_items_device_wm; 19, additive: inter-intra prediction:
 * SvtGpuInterIntraBlock, svtgpu_interintra_predict_batch, svtgpu_interintra_mode_sse_batch, svtgpu_interintra_smooth_mask, the
 * two svtgpu_aom_(highbd_)blend_a64_mask shims and the two svtgpu_aom_(highbd_)intra_predictor shims -- new entries and a new
 * struct only, so no bump).
 * A caller built against another header checks svtgpu_abi_version() ==
 * SVTGPU_ABI_VERSION once at start-up and refuses to run on a mismatch. */
#define SVTGPU_ABI_VERSION 19
int32_t     svtgpu_abi_version(void);
const char *svtgpu_error_string(int code);

typedef struct SvtGpuContext SvtGpuContext;
/* One context per (process, device). Owns a HIP stream and the scratch of the frame-level calls. */
int   svtgpu_context_create(int device, SvtGpuContext **out);
void  svtgpu_context_destroy(SvtGpuContext *ctx);
void *svtgpu_context_stream(SvtGpuContext *ctx); /* the context's hipStream_t */
int   svtgpu_synchronize(SvtGpuContext *ctx, void *stream);
/* A stream for the frame-level calls (a hipStream_t; priority > 0 the device's highest, < 0 its lowest, 0 normal).
 * Each stream is one hardware queue while the process has no more streams than GPU_MAX_HW_QUEUES; past that, streams
 * share queues and a frame's chain waits behind another's.  An encoder running several pictures at once creates its
 * per-picture streams here (or otherwise exactly as many as it runs), not from a framework's stream pool (round 6:
 * torch.cuda.Stream()'s pool of 32 streams per priority cost 1080p 10-bit at four frames in flight 23%). */
int  svtgpu_stream_create(SvtGpuContext *ctx, int32_t priority, void **out_stream);
void svtgpu_stream_destroy(void *stream);
/* Plain device buffers for the pointer-level entry points (CCSO, svtgpu_convert_plane, ...) when the caller has no
 * allocator of its own; upload / download are complete when they return (the stream is synchronized). */
int  svtgpu_buffer_alloc(SvtGpuContext *ctx, size_t bytes, void **dev_out);
void svtgpu_buffer_free(void *dev);
int  svtgpu_buffer_upload(void *dev, const void *host, size_t bytes, void *stream);
int  svtgpu_buffer_download(void *host, const void *dev, size_t bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident 4:2:0 pictures
 *   Samples are uint8 when bit_depth == 8 and uint16 when bit_depth == 10 (the reference's
 *   "16-bit pipeline", EbEncHandle.c:4534).  width/height are luma sizes, multiples of 8.
 *   Plane p (0=Y,1=U,2=V) is stored with stride svtgpu_frame_stride(f, p) samples and no padding
 *   requirement on the caller side.
 * ------------------------------------------------------------------------------------------- */
typedef struct SvtGpuFrame SvtGpuFrame;
int      svtgpu_frame_create(SvtGpuContext *ctx, int32_t width, int32_t height, int32_t bit_depth,
                             SvtGpuFrame **out);
void     svtgpu_frame_destroy(SvtGpuFrame *f);
int32_t  svtgpu_frame_stride(const SvtGpuFrame *f, int plane);
void    *svtgpu_frame_plane_ptr(SvtGpuFrame *f, int plane); /* device pointer */
/* host <-> device copies of one plane; host_stride in samples. Asynchronous on `stream` unless the
 * host buffer is pageable (then HIP makes it synchronous). */
int svtgpu_frame_upload(SvtGpuFrame *f, int plane, const void *host, int32_t host_stride, void *stream);
int svtgpu_frame_download(const SvtGpuFrame *f, int plane, void *host, int32_t host_stride, void *stream);
/* Only the samples of rect = {x0, y0, x1, y1} (plane coordinates) of one plane; `host` is the plane's origin as for
 * svtgpu_frame_upload.  A rank of a tiled picture uploads its SvtGpuTilePlan::in_rect (chroma halved, outward). */
int svtgpu_frame_upload_rect(SvtGpuFrame *f, int plane, const void *host, int32_t host_stride, const int32_t rect[4],
                             void *stream);
int svtgpu_frame_copy(SvtGpuFrame *dst, const SvtGpuFrame *src, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A picture tiled over several GPUs (BASELINE.json config 4).  No reference counterpart: the
 * reference splits a picture into segments for its worker threads (cdef_seg_search / restoration_seg_search per
 * segment, EbEncHandle.c:503-514) and gathers their results under a mutex (EbCdefProcess.c:406, EbRestProcess.c:614).
 * Here each rank (one process per GPU) takes a tile, and the frame-level calls exchange what the reference's
 * gather hands to its sequential finish: the DLF trial SSEs, the CDEF search tables and the LR search records.
 * ------------------------------------------------------------------------------------------- */
#define SVTGPU_COMM_ID_BYTES 128
typedef struct SvtGpuComm SvtGpuComm;
/* RCCL over xGMI: rank 0 creates the id, the caller broadcasts its bytes (any transport), every rank creates its
 * communicator on its device.  One communicator per frame in flight. */
int svtgpu_comm_unique_id(uint8_t id[SVTGPU_COMM_ID_BYTES]);
int svtgpu_comm_create(SvtGpuContext *ctx, int32_t nranks, int32_t rank, const uint8_t id[SVTGPU_COMM_ID_BYTES],
                       SvtGpuComm **out);
/* svtgpu_comm_create with a bounded init: the communicator is created non-blocking (ncclCommInitRankConfig, blocking
 * = 0) and polled against timeout_ms (0: the default deadline, SVTGPU_COMM_TIMEOUT_MS or 60000 ms).  A peer that never
 * joins (it died between the id broadcast and its init) returns SVTGPU_ERR_HIP within the deadline with
 * svtgpu_error_string naming "communicator init", the frame slot `slot`, this rank and the rank count; the partial
 * communicator is aborted.  svtgpu_comm_create = this with timeout_ms 0 and slot -1.  SVTGPU_COMM_INIT=blocking
 * restores the blocking ncclCommInitRank. */
int svtgpu_comm_create_bounded(SvtGpuContext *ctx, int32_t nranks, int32_t rank, const uint8_t id[SVTGPU_COMM_ID_BYTES],
                               int32_t timeout_ms, int32_t slot, SvtGpuComm **out);
/* A caller-supplied host transport (e.g. MPI or gloo): allreduce_u64 sums n uint64 element-wise over the ranks in
 * place (every rank receives the sums) and returns 0.  Device buffers are staged through pinned host memory.  For
 * rehearsals on CPUs and for several ranks on one GPU (RCCL needs one rank per device). */
typedef struct SvtGpuHostTransport {
    void *user;
    int (*allreduce_u64)(void *user, uint64_t *buf, size_t n);
} SvtGpuHostTransport;
int     svtgpu_comm_create_host(int32_t nranks, int32_t rank, const SvtGpuHostTransport *t, SvtGpuComm **out);
void    svtgpu_comm_destroy(SvtGpuComm *c);
int32_t svtgpu_comm_nranks(const SvtGpuComm *c);
int32_t svtgpu_comm_rank(const SvtGpuComm *c);
/* element-wise sum of n uint64 over the ranks, in place; on_device: buf is device memory (enqueued on `stream` with
 * RCCL), else host memory (synchronous) */
int svtgpu_comm_allreduce_u64(SvtGpuComm *c, void *buf, size_t n, int32_t on_device, void *stream);
/* Every exchange is bounded by the communicator's deadline (default 60000 ms, SVTGPU_COMM_TIMEOUT_MS overrides it).
 * A frame-level call whose exchange does not complete in time (a peer rank skipped it, or failed before reaching it)
 * returns SVTGPU_ERR_HIP, svtgpu_error_string names the exchange ("DLF trial SSEs", "CDEF search tables", "LR search
 * records"), the frame slot and the exchange's sequence number; an RCCL communicator is aborted (ncclCommAbort ends
 * this rank's pending collectives) and the communicator fails every later call (svtgpu_comm_failed).  A host
 * transport bounds its own wait by svtgpu_comm_timeout_ms and returns non-zero when it expires. */
int     svtgpu_comm_set_timeout(SvtGpuComm *c, int32_t timeout_ms);
int32_t svtgpu_comm_timeout_ms(const SvtGpuComm *c);
int     svtgpu_comm_set_slot(SvtGpuComm *c, int32_t frame_slot); /* the frame slot named in a timeout's message */
int32_t svtgpu_comm_failed(const SvtGpuComm *c);
/* host wait for `stream`, bounded by the deadline when one of the communicator's device-side exchanges (enqueued
 * without a host wait: svtgpu_comm_allreduce_u64 on device memory) was enqueued on `stream` since its last completed
 * wait -- the whole wait is then bounded (per-exchange completion markers lengthened a tiled rank's latency chains
 * by 7 %), so work queued behind an exchange counts against the deadline too */
int     svtgpu_comm_sync(SvtGpuComm *c, void *stream);
/* the number of per-block RTCD shim calls this process made (each runs on the process-wide default context): evidence
 * that an encoder with the shims installed really ran its kernels on the device */
uint64_t svtgpu_shim_calls(void);
/* test support: holds `stream` busy for `ms` milliseconds (<= 10000) with one spinning wave */
int     svtgpu_debug_stall(SvtGpuContext *ctx, void *stream, int32_t ms);

/* The tiles of a gx x gy split of a width x height picture and what rank `rank` (row-major) computes.  Tile edges
 * fall on the luma restoration-unit grid (unit_size[0], a multiple of 64: also filter-block and superblock edges), so
 * each rank's loop-restoration units lie in its own part of the frame:
 *   tile       {x0, y0, x1, y1} luma: the rank's share of the DLF trial SSEs (a partition of the frame);
 *   fb_rect    {col0, row0, col1, row1}: the 64x64 CDEF filter blocks it searches (a partition);
 *   lr_units   per plane {col0, row0, col1, row1} unit indices it searches (a partition of each plane's units);
 *   lr_out     per plane {x0, y0, x1, y1} plane samples: the union of those units, the part of the final picture the
 *              rank produces (a partition);
 *   cdef_out   {x0, y0, x1, y1} luma: the CDEF output its LR search and apply read (lr_out plus an 8-sample apron);
 *   dlf_out    {x0, y0, x1, y1} luma: the DLF output its CDEF search / apply and LR boundary lines read (its tile and
 *              lr_out plus a 16-sample apron);
 *   in_rect    {x0, y0, x1, y1} luma: the recon and source samples the rank's calls read (dlf_out plus the deblocking
 *              filter's 16-sample reach): what a rank uploads of each input picture.
 * Host only.  SVTGPU_ERR_INVALID_ARG when some rank would get no unit. */
typedef struct SvtGpuTilePlan {
    int32_t tile[4], fb_rect[4], lr_units[3][4], lr_out[3][4], cdef_out[4], dlf_out[4], in_rect[4];
} SvtGpuTilePlan;
int svtgpu_tile_plan(int32_t width, int32_t height, const int32_t unit_size[3], int32_t gx, int32_t gy, int32_t rank,
                     SvtGpuTilePlan *out);
/* The same for a picture of sb_size (64 or 128) superblocks: with 128 the tile edges are also multiples of 128, so no
 * 128x128 CDEF area is cut (svtgpu_tile_plan = sb_size 64). */
int svtgpu_tile_plan_sb(int32_t width, int32_t height, const int32_t unit_size[3], int32_t sb_size, int32_t gx,
                        int32_t gy, int32_t rank, SvtGpuTilePlan *out);
/* A picture whose crop size (frm_size.frame_width x frame_height, the area loop restoration covers) is below its
 * 8-aligned coded size (width x height: the deblocking / CDEF frames, coded - crop < 8 each way): the restoration
 * units tile the crop (chroma rounded up), the tiles keep their edges on the luma unit grid and the last tile runs to
 * the coded edge.  Each rank's LR state is created with the crop size and its DLF state told the crop
 * (svtgpu_dlf_set_crop), as on one GPU.  svtgpu_tile_plan_sb = crop equal to the coded size. */
int svtgpu_tile_plan_crop(int32_t width, int32_t height, int32_t crop_w, int32_t crop_h, const int32_t unit_size[3],
                          int32_t sb_size, int32_t gx, int32_t gy, int32_t rank, SvtGpuTilePlan *out);

/* ---------------------------------------------------------------------------------------------
 * CDEF — per-block RTCD shims (host pointers, synchronous)
 * ------------------------------------------------------------------------------------------- */
/* replaces svt_aom_cdef_find_dir (common_dsp_rtcd.h:1017); C: EbCdef.c:150 */
uint8_t svtgpu_cdef_find_dir(const uint16_t *img, int32_t stride, int32_t *var, int32_t coeff_shift);
/* replaces svt_aom_cdef_find_dir_dual (common_dsp_rtcd.h:1096); C: EbCdef.c:212 */
void svtgpu_cdef_find_dir_dual(const uint16_t *img1, const uint16_t *img2, int stride, int32_t *var1,
                               int32_t *var2, int32_t coeff_shift, uint8_t *out1, uint8_t *out2);
/* replaces svt_cdef_filter_block (common_dsp_rtcd.h:1099); C: EbCdef.c:253.
 * `in` points into a CDEF_BSTRIDE(=144)-stride buffer; rows -2..h+1 and cols -2..w+1 are read. */
void svtgpu_cdef_filter_block(uint8_t *dst8, uint16_t *dst16, int32_t dstride, const uint16_t *in,
                              int32_t pri_strength, int32_t sec_strength, int32_t dir, int32_t pri_damping,
                              int32_t sec_damping, int32_t bsize, int32_t coeff_shift,
                              uint8_t subsampling_factor);
/* replaces svt_compute_cdef_dist_16bit / _8bit (aom_dsp_rtcd.h:62-64); C: EbEncCdef.c:129/175 */
uint64_t svtgpu_compute_cdef_dist_16bit(const uint16_t *dst, int32_t dstride, const uint16_t *src,
                                        const SVTGPU_CDEF_LIST_T *dlist, int32_t cdef_count, SVTGPU_BLOCK_SIZE_T bsize,
                                        int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);
uint64_t svtgpu_compute_cdef_dist_8bit(const uint8_t *dst8, int32_t dstride, const uint8_t *src8,
                                       const SVTGPU_CDEF_LIST_T *dlist, int32_t cdef_count, SVTGPU_BLOCK_SIZE_T bsize,
                                       int32_t coeff_shift, int32_t pli, uint8_t subsampling_factor);
/* replaces svt_search_one_dual (aom_dsp_rtcd.h:239); C: EbEncCdef.c:627 */
uint64_t svtgpu_search_one_dual(int *lev0, int *lev1, int nb_strengths, uint64_t **mse[2], int sb_count,
                                int start_gi, int end_gi);
/* replaces svt_cdef_filter_block_8xn_16 (common_dsp_rtcd.h:1100; AVX2 only in the reference,
 * cdef_block_avx2.c:463): an 8-wide luma block, rows 0, s, 2s, ... (s = subsampling_factor) of `height`, into a
 * uint16 dst; `in` points into a CDEF_BSTRIDE(=144)-stride buffer, pri_strength already adjusted */
void svtgpu_cdef_filter_block_8xn_16(const uint16_t *const in, const int32_t pri_strength, const int32_t sec_strength,
                                     const int32_t dir, int32_t pri_damping, int32_t sec_damping,
                                     const int32_t coeff_shift, uint16_t *const dst, const int32_t dstride,
                                     uint8_t height, uint8_t subsampling_factor);
/* replaces svt_aom_copy_rect8_8bit_to_16bit (common_dsp_rtcd.h:1105; C EbCdef.c:303): the 8-bit -> 16-bit
 * staging copy of the CDEF input buffer, v rows x h columns */
void svtgpu_aom_copy_rect8_8bit_to_16bit(uint16_t *dst, int32_t dstride, const uint8_t *src, int32_t sstride, int32_t v,
                                         int32_t h);

/* ---------------------------------------------------------------------------------------------
 * CDEF — frame level (device-resident)
 * ------------------------------------------------------------------------------------------- */
#define SVTGPU_CDEF_TOTAL_STRENGTHS 64
#define SVTGPU_CDEF_MAX_STRENGTHS 16

/* Subset of the reference's CdefControls (EbPictureControlSet.h:592-628) that the search and pick
 * read.  Strength codes are pri*4 + sec (sec code 3 means strength 4), as in
 * EncModeConfig.c:860-1330. */
typedef struct SvtGpuCdefControls {
    uint8_t  first_pass_fs_num;
    uint8_t  default_second_pass_fs_num;
    uint8_t  default_first_pass_fs[SVTGPU_CDEF_TOTAL_STRENGTHS];
    uint8_t  default_second_pass_fs[SVTGPU_CDEF_TOTAL_STRENGTHS];
    int8_t   default_first_pass_fs_uv[SVTGPU_CDEF_TOTAL_STRENGTHS];  /* -1 = chroma not tested */
    int8_t   default_second_pass_fs_uv[SVTGPU_CDEF_TOTAL_STRENGTHS]; /* -1 = chroma not tested */
    uint8_t  subsampling_factor;                                     /* 1, 2 or 4 */
    uint16_t zero_fs_cost_bias;                                      /* 0 = off, else x/64 */
    /* use_reference_cdef_fs levels (11, 14, 15, 17): no strength search; the frame uses the strength pair the
     * mode-decision configuration predicted from the references (pred_y_f / pred_uv_f, strength codes 0..63,
     * set by the caller as EbModeDecisionConfigurationProcess.c:765-840 does) */
    int8_t   use_reference_cdef_fs;
    int8_t   pred_y_f;
    int8_t   pred_uv_f;
} SvtGpuCdefControls;

/* Fill `c` exactly as set_cdef_controls(cdef_level) does (EncModeConfig.c:860-1330), levels 1..17
 * (pred_y_f / pred_uv_f left 0). Returns SVTGPU_ERR_UNSUPPORTED for level 0 (CDEF off).
 * fast_decode/resolution tweaks of the zero_fs_cost_bias are applied by the caller. */
int svtgpu_cdef_controls_for_level(int cdef_level, SvtGpuCdefControls *c);

/* Frame parameters chosen by the pick; layout mirrors CdefParams (EbAv1Structs.h:359-369). */
typedef struct SvtGpuCdefParams {
    uint8_t cdef_damping;
    uint8_t cdef_bits;
    uint8_t cdef_y_strength[SVTGPU_CDEF_MAX_STRENGTHS];
    uint8_t cdef_uv_strength[SVTGPU_CDEF_MAX_STRENGTHS];
} SvtGpuCdefParams;

/* Device-resident search state for one frame (mse_seg, skip_cdef_seg and cdef_dir_data of the
 * reference's PictureControlSet, EbPictureControlSet.h:268-270). */
typedef struct SvtGpuCdefFrameState SvtGpuCdefFrameState;
int  svtgpu_cdef_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, SvtGpuCdefFrameState **out);
void svtgpu_cdef_state_destroy(SvtGpuCdefFrameState *s);
int32_t svtgpu_cdef_state_nfb(const SvtGpuCdefFrameState *s); /* nvfb*nhfb */

/* Per-8x8 "filter this block" mask, row-major, ((h+7)/8) x ((w+7)/8) bytes; an 8x8 block is
 * listed iff any of its four 4x4 mode-info units is non-skip (svt_sb_compute_cdef_list,
 * EbEncCdef.c:238).  Upload once per frame; NULL mask = every block listed. */
int svtgpu_cdef_set_block_mask(SvtGpuCdefFrameState *s, const uint8_t *host_mask, void *stream);

/* SB128 mode info: the BlockSize (EbDefinitions.h enum; 13 = 64X128, 14 = 128X64, 15 = 128X128) of the mode
 * info at each 64x64 filter block's top-left, nfb bytes row-major — what cdef_seg_search and finish_cdef_search
 * read (EbCdefProcess.c:188-199, EbEncCdef.c:805-812).  The search then folds each 128-wide area into its top-left
 * filter block and the pick copies the area's strength into the other halves.  NULL = 64x64 superblocks.
 * With frame bands (svtgpu_cdef_set_fb_rows) the band edges must fall on even filter-block rows. */
int svtgpu_cdef_set_fb_bsize(SvtGpuCdefFrameState *s, const uint8_t *fb_bsize, void *stream);

/* ≙ all segments of cdef_seg_search (EbCdefProcess.c:114-357).  recon = DLF output, source = input picture
 * (same geometry/bit depth).  With use_reference_cdef_fs no strength is searched (EbCdefProcess.c:400): only
 * the per-8x8 directions/variances the apply needs are computed (svt_av1_cdef_frame finds them itself then,
 * EbEncCdef.c:403), and the mse table is zeroed. */
int svtgpu_cdef_search_frame(SvtGpuCdefFrameState *s, const SvtGpuFrame *recon, const SvtGpuFrame *source,
                             const SvtGpuCdefControls *ctrls, int32_t base_q_idx, void *stream);

/* ≙ finish_cdef_search (EbEncCdef.c:728-926) with svt_search_one_dual on the device; with
 * use_reference_cdef_fs its first branch (:744-789): one strength pair {pred_y_f, pred_uv_f}, index 0 everywhere.
 * lambda = full_lambda of the frame (computed by the encoder's lambda function table).
 * Writes params and the per-FB strength index (int8 per FB, host array of nfb entries) and keeps
 * the per-FB index on the device for svtgpu_cdef_apply_frame.  Synchronous (returns host data).  It hands the
 * parameters to the caller only: the device parameters of an earlier svtgpu_cdef_pick_async are dropped, so
 * svtgpu_cdef_apply_frame(params = NULL) and svtgpu_cdef_read_params return SVTGPU_ERR_INVALID_ARG until the next
 * svtgpu_cdef_pick_async. */
int svtgpu_cdef_pick(SvtGpuCdefFrameState *s, const SvtGpuCdefControls *ctrls, int32_t base_q_idx,
                     uint64_t lambda, SvtGpuCdefParams *params_out, int8_t *fb_strength_out, void *stream);

/* The same pick with no host wait (round 6): the settle check's outcome reaches the later strength-search steps
 * through device memory (they exit at once when every chain has settled), and the RD choice leaves the frame
 * parameters and the per-FB indices in device memory, where svtgpu_cdef_apply_frame(params = NULL) reads them --
 * everything in stream order.  svtgpu_cdef_read_params returns them (after a bounded wait for `stream`) once the
 * caller needs them on the host, e.g. to write the frame header. */
int svtgpu_cdef_pick_async(SvtGpuCdefFrameState *s, const SvtGpuCdefControls *ctrls, int32_t base_q_idx,
                           uint64_t lambda, void *stream);
int svtgpu_cdef_read_params(SvtGpuCdefFrameState *s, SvtGpuCdefParams *params_out, int8_t *fb_strength_out,
                            void *stream);

/* Optional override of the per-FB strength index used by apply (host array of nfb entries). */
int svtgpu_cdef_set_fb_strength(SvtGpuCdefFrameState *s, const int8_t *fb_strength, void *stream);

/* ≙ svt_av1_cdef_frame (EbEncCdef.c:284-610): apply params to `recon` (DLF output) and write the
 * filtered picture to `out` (out-of-place; the reference's in-place result with its saved
 * unfiltered line/column buffers is identical).  Uses dir/var of the last search.  params == NULL: the parameters
 * of the last svtgpu_cdef_pick_async, read from device memory in stream order -- with nothing in between: no
 * asynchronous pick yet, or a svtgpu_cdef_pick on the state since, is SVTGPU_ERR_INVALID_ARG. */
int svtgpu_cdef_apply_frame(SvtGpuCdefFrameState *s, const SvtGpuFrame *recon, SvtGpuFrame *out,
                            const SvtGpuCdefParams *params, void *stream);

/* Frame tiling across GPUs (BASELINE config 4): restrict search and apply to filter-block rows
 * [fb_row_begin, fb_row_end).  Samples outside the band are still read as filter context (apron), so
 * the picture passed in must hold valid samples for the band +-3 rows.  Default: all rows. */
int svtgpu_cdef_set_fb_rows(SvtGpuCdefFrameState *s, int32_t fb_row_begin, int32_t fb_row_end);
/* A picture tiled over GPUs (svtgpu_tile_plan): the search covers the filter blocks of fb_rect = {col0, row0, col1,
 * row1} only and leaves zeros elsewhere in the tables; svtgpu_cdef_pick first sums the mse / skip / dir / var tables
 * over `comm` (one contributor per entry: the gather of every rank's blocks; the pick is then the same on every rank;
 * the sums run once per search: a second pick on the same search reads the gathered tables); the apply writes only the luma rectangle out_rect = {x0, y0, x1, y1} (chroma halved, rounded outward), reading
 * the DLF output 2 samples around it.  NULL rects: the whole frame; NULL comm: no exchange. */
int svtgpu_cdef_set_tile(SvtGpuCdefFrameState *s, const int32_t fb_rect[4], const int32_t out_rect[4],
                         SvtGpuComm *comm);
/* Use caller-owned device memory for the search tables: mse [2][nfb][64] uint64 and skip [nfb] uint8
 * (e.g. buffers all-reduced with RCCL between the search and the pick).  NULL, NULL restores the
 * state's own buffers.  svtgpu_cdef_clear_tables zeroes both (a band search then leaves zeros —
 * the identity of an all-reduce-sum — outside its rows).  The library touches exactly nfb bytes of a
 * bound skip table (the tiled pick sums it through a padded copy of its own). */
int svtgpu_cdef_bind_tables(SvtGpuCdefFrameState *s, void *mse_dev, void *skip_dev);
/* The same for the per-8x8 direction/variance tables the apply reuses: dir [nfb][64] uint8, var [nfb][64]
 * int32 (zero outside a band after svtgpu_cdef_clear_tables, so an all-reduce-sum completes them and every
 * rank can apply the whole frame). */
int svtgpu_cdef_bind_dir_tables(SvtGpuCdefFrameState *s, void *dir_dev, void *var_dev);
/* zeroes mse, skip, dir and var */
int svtgpu_cdef_clear_tables(SvtGpuCdefFrameState *s, void *stream);

/* Host views of the search results (synchronous). mse: [2][nfb][64] uint64, skip: [nfb] uint8,
 * dir: [nfb][64] uint8 and var: [nfb][64] int32 (8x8 blocks of the FB, row-major). Any may be NULL. */
int svtgpu_cdef_read_state(SvtGpuCdefFrameState *s, uint64_t *mse, uint8_t *skip, uint8_t *dir, int32_t *var,
                           void *stream);
/* Device pointer of the [2][nfb][64] uint64 mse table (for RCCL gathers across tiles). */
void *svtgpu_cdef_mse_device_ptr(SvtGpuCdefFrameState *s);

/* ---------------------------------------------------------------------------------------------
 * Deblocking loop filter — per-segment RTCD shims (host pointers, synchronous).
 * Each filters one 4-sample edge segment exactly like the reference C (EbDeblockingCommon.c).
 * ------------------------------------------------------------------------------------------- */
/* replace svt_aom_lpf_{horizontal,vertical}_{4,6,8,14} (common_dsp_rtcd.h:1116-1131) */
void svtgpu_lpf_horizontal_4(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                             const uint8_t *thresh);
void svtgpu_lpf_horizontal_6(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                             const uint8_t *thresh);
void svtgpu_lpf_horizontal_8(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                             const uint8_t *thresh);
void svtgpu_lpf_horizontal_14(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                              const uint8_t *thresh);
void svtgpu_lpf_vertical_4(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                           const uint8_t *thresh);
void svtgpu_lpf_vertical_6(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                           const uint8_t *thresh);
void svtgpu_lpf_vertical_8(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                           const uint8_t *thresh);
void svtgpu_lpf_vertical_14(uint8_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                            const uint8_t *thresh);
/* replace svt_aom_highbd_lpf_{horizontal,vertical}_{4,6,8,14} (common_dsp_rtcd.h:1132-1146) */
void svtgpu_highbd_lpf_horizontal_4(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                    const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_horizontal_6(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                    const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_horizontal_8(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                    const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_horizontal_14(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                     const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_vertical_4(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                  const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_vertical_6(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                  const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_vertical_8(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                  const uint8_t *thresh, int32_t bd);
void svtgpu_highbd_lpf_vertical_14(uint16_t *s, int32_t pitch, const uint8_t *blimit, const uint8_t *limit,
                                   const uint8_t *thresh, int32_t bd);

/* ---------------------------------------------------------------------------------------------
 * Deblocking loop filter — frame level (device-resident, in place)
 * ------------------------------------------------------------------------------------------- */
/* One record per 4x4 mode-info unit (mi), raster order, mi_rows x mi_cols (mi = 4 luma samples;
 * frame dimensions rounded up to 8).  The MbModeInfo fields set_lpf_parameters reads
 * (EbDeblockingFilter.c:162-282); values are the reference's enums (BlockSize, PredictionMode,
 * MvReferenceFrame with INTRA_FRAME = 0). */
typedef struct SvtGpuLfMi {
    uint8_t bsize;      /* block_mi.bsize */
    uint8_t tx_depth;   /* block_mi.tx_depth (0..2) */
    uint8_t skip;       /* block_mi.skip */
    int8_t  ref_frame0; /* block_mi.ref_frame[0] */
    uint8_t mode;       /* block_mi.mode */
    uint8_t segment_id; /* block_mi.segment_id */
    uint8_t pad[2];
} SvtGpuLfMi;

/* Frame loop-filter parameters: struct LoopFilter (EbDefinitions.h:1903-1920) + the segmentation
 * feature arrays (EbSegmentationParams.h:49-53) the level table depends on.  delta_lf is not
 * supported (delta_lf_present = 0). */
typedef struct SvtGpuLfParams {
    int32_t filter_level[2]; /* luma: [0] vertical edges, [1] horizontal edges */
    int32_t filter_level_u;
    int32_t filter_level_v;
    int32_t sharpness_level;
    uint8_t mode_ref_delta_enabled;
    int8_t  ref_deltas[8];
    int8_t  mode_deltas[2];
    uint8_t segmentation_enabled;
    int16_t seg_feature_data[8][8];    /* [segment][SEG_LVL_*] */
    int16_t seg_feature_enabled[8][8]; /* [segment][SEG_LVL_*] */
} SvtGpuLfParams;

typedef struct SvtGpuDlfState SvtGpuDlfState;
int  svtgpu_dlf_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, SvtGpuDlfState **out);
void svtgpu_dlf_state_destroy(SvtGpuDlfState *s);
/* upload the mi grid ((h+7)/8*2 rows x (w+7)/8*2 cols records): asynchronous on `stream` through pinned staging,
 * the caller may reuse its buffer on return (one grid per frame) */
int svtgpu_dlf_set_mode_info(SvtGpuDlfState *s, const SvtGpuLfMi *mi, void *stream);
/* the same from a grid already in device memory (`d_mi`, same layout; e.g. written by a device mode decision):
 * copied in stream order (the caller may overwrite `d_mi` once `stream` has passed this call), no host pass and no
 * PCIe.  The records kernel checks the fields; a grid with records out of range is clamped and reported as
 * SVTGPU_ERR_INVALID_ARG by the next svtgpu_dlf_pick, or by the next svtgpu_dlf_frame(_to) when no pick ran (the
 * FROM_Q levels); each upload is judged on its own. */
int svtgpu_dlf_set_mode_info_device(SvtGpuDlfState *s, const SvtGpuLfMi *d_mi, void *stream);
/* The picture's unpadded size when it is off the 8-sample grid (scs->max_input_luma_width - max_input_pad_right,
 * _height - _pad_bottom; EbDeblockingFilter.c:99-129): set_lpf_parameters filters no edge at or past it in a plane
 * (luma crop_width x crop_height, chroma both >> 1; :173-178), while the frames and the mode-info grid stay the
 * 8-aligned coded size the state was created with.  Default: the coded size.  Takes effect at the next
 * svtgpu_dlf_set_mode_info(_device). */
int svtgpu_dlf_set_crop(SvtGpuDlfState *s, int32_t crop_width, int32_t crop_height);
/* ≙ svt_av1_loop_filter_frame(frame, pcs, plane_start, plane_end) (EbDeblockingFilter.c:624-653):
 * all vertical edges of each plane, then all horizontal edges (equivalent to the reference's
 * SB-lagged order with combine_vert_horz_lf = 1, :41, :580-605), in place on `frame`. */
int svtgpu_dlf_frame(SvtGpuDlfState *s, SvtGpuFrame *frame, const SvtGpuLfParams *params, int32_t plane_start,
                     int32_t plane_end, void *stream);
/* Out-of-place form of svtgpu_dlf_frame: reads `in`, writes every sample of planes
 * [plane_start, plane_end) of `out` (filtered, or copied when the plane is not filtered). */
int svtgpu_dlf_frame_to(SvtGpuDlfState *s, const SvtGpuFrame *in, SvtGpuFrame *out, const SvtGpuLfParams *params,
                        int32_t plane_start, int32_t plane_end, void *stream);
/* ≙ svt_av1_pick_filter_level(LPF_PICK_FROM_FULL_IMAGE) (EbDeblockingFilter.c:1129-1252): bisection
 * on the filter level per plane with a device trial per level (filter + SSE vs `source` + restore).
 * `params` carries the previous levels in and the picked levels out; `recon` is left unfiltered.
 * dlf_avg_uv/temporal_layer_index select the reference's "use averaged chroma levels" shortcut.
 * Synchronous.  The levels go to the caller only: the device levels of an earlier svtgpu_dlf_pick_async are dropped,
 * so svtgpu_dlf_frame(_to)(..., params = NULL, ...) and svtgpu_dlf_read_levels return SVTGPU_ERR_INVALID_ARG until
 * the next svtgpu_dlf_pick_async. */
int svtgpu_dlf_pick(SvtGpuDlfState *s, SvtGpuFrame *recon, const SvtGpuFrame *source, SvtGpuLfParams *params,
                    int32_t dlf_avg, int32_t dlf_avg_uv, int32_t temporal_layer_index,
                    int32_t early_exit_convergence, int32_t tx_mode_only_4x4, void *stream);
/* The same level search with no host wait (≙ svt_av1_pick_filter_level, LPF_PICK_FROM_FULL_IMAGE): the bisection of
 * search_filter_level (EbDeblockingFilter.c:886-991) runs on the device -- every trial round's last workgroup takes the
 * step, a final one-workgroup kernel completes a search still open after the rounds enqueued (sized from the previous
 * search) -- and the picked levels stay there.  `params` carries the previous levels in (read at the call).
 * svtgpu_dlf_frame(_to)(..., params = NULL, ...) then filters with the picked levels in stream order, and
 * svtgpu_dlf_read_levels waits for them (the frame header's levels).  The NULL form refers to the last
 * svtgpu_dlf_pick_async with no svtgpu_dlf_pick on the state since.  A picture tiled over GPUs runs the synchronous
 * search here and keeps its levels. */
int svtgpu_dlf_pick_async(SvtGpuDlfState *s, const SvtGpuFrame *recon, const SvtGpuFrame *source,
                          const SvtGpuLfParams *params, int32_t dlf_avg, int32_t dlf_avg_uv,
                          int32_t temporal_layer_index, int32_t early_exit_convergence, int32_t tx_mode_only_4x4,
                          void *stream);
/* Waits for the last svtgpu_dlf_pick_async of `s` on `stream` and returns its parameters (the input parameters with
 * the picked levels; sharpness 0).  SVTGPU_ERR_INVALID_ARG: no asynchronous pick ran, or the device mode-info grid it
 * used had records out of range. */
int svtgpu_dlf_read_levels(SvtGpuDlfState *s, SvtGpuLfParams *params_out, void *stream);
/* measurement: the trial rounds the last collected asynchronous search took, and the rounds the last one enqueued
 * (a search needing more is completed by the finish kernel, one workgroup: far slower) */
int svtgpu_dlf_async_rounds(const SvtGpuDlfState *s, int32_t *taken, int32_t *enqueued);
/* A picture tiled over GPUs (svtgpu_tile_plan): the level search measures each trial's SSE over the luma
 * rectangle sse_rect = {x0, y0, x1, y1} (the rank's tile; chroma halved) and sums it over `comm` before every
 * bisection step, so every rank takes the same steps; svtgpu_dlf_frame(_to) writes only out_rect (chroma halved,
 * rounded outward), reading the input 12 samples around it.  Rect edges are multiples of 8 (or the frame edge).
 * NULL rects: the whole frame; NULL comm: no exchange. */
int svtgpu_dlf_set_tile(SvtGpuDlfState *s, const int32_t sse_rect[4], const int32_t out_rect[4], SvtGpuComm *comm);
/* LPF_PICK_FROM_Q: the loop-filter levels from the quantizer, no search (host only, no device work).
 * ≙ svt_av1_pick_filter_level_by_q (EbDeblockingFilter.c:1036-1125), the path svt_av1_pick_filter_level takes
 * for method >= LPF_PICK_FROM_Q (:1139-1146; the SB-based DLF levels 3..5).  Inputs are the fields it reads:
 * the sequence bit depth, base_q_idx, the frame / slice type, the two temporal layer indices it uses
 * (PictureControlSet's for the zero-strength threshold, the parent's for the reference-off rule), the input
 * resolution class (ResolutionRange 0..6), DlfCtrls.zero_filter_strength_lvl, the per-64x64 ME distortions
 * (rc_me_distortion, b64_count of them), and the loop-filter levels {y0, y1, u, v} of each SINGLE reference in
 * ref_frame_type_arr (compound pairs are skipped by the reference; nref = 0 for none). */
typedef struct SvtGpuDlfByQ {
    int32_t         bit_depth;                 /* 8, 10 or 12 */
    int32_t         base_q_idx;                /* 0..255 */
    int32_t         frame_type;                /* KEY_FRAME = 0 */
    int32_t         slice_type;                /* B_SLICE 0, P_SLICE 1, I_SLICE 2 */
    int32_t         temporal_layer_index;      /* pcs->temporal_layer_index */
    int32_t         ppcs_temporal_layer_index; /* pcs->ppcs->temporal_layer_index */
    int32_t         input_resolution;          /* 0..6 */
    int32_t         zero_filter_strength_lvl;  /* 0..3 */
    int32_t         b64_count;
    const uint32_t *me_sad;                    /* b64_count entries */
    int32_t         nref;                      /* 0..7 */
    int32_t         ref_levels[7][4];          /* {filter_level[0], filter_level[1], filter_level_u, filter_level_v} */
} SvtGpuDlfByQ;
int svtgpu_dlf_pick_by_q(const SvtGpuDlfByQ *in, int32_t filter_level[4]);
/* ≙ qp_based_dlf_param (EbDeblockingFilter.c:992-1031): luma / chroma level guesses from base_q_idx */
int svtgpu_dlf_qp_based_param(int32_t bit_depth, int32_t base_q_idx, int32_t frame_type, int32_t *filter_level_y,
                              int32_t *filter_level_uv);

/* Σ (a - b)^2 over one plane (svt_spatial_full_distortion_kernel / svt_full_distortion_kernel16_bits
 * over the frame, EbDeblockingFilter.c:716-838). Synchronous. */
int svtgpu_plane_sse(const SvtGpuFrame *a, const SvtGpuFrame *b, int32_t plane, uint64_t *sse, void *stream);


/* =========================================================================================
 * Mode-decision distortion: SAD / SSE / variance
 * ========================================================================================= */
/* RTCD-compatible per-block shims, one per AV1 block size (BlockSize order).  Synchronous.
 *   svtgpu_aom_sad{W}x{H}              ≙ svt_aom_sad{W}x{H}            (aom_dsp_rtcd.h:264-350, C EbComputeSAD_C.c:117-206)
 *   svtgpu_aom_sad{W}x{H}x4d           ≙ svt_aom_sad{W}x{H}x4d
 *   svtgpu_aom_variance{W}x{H}         ≙ svt_aom_variance{W}x{H}       (aom_dsp_rtcd.h:480-540, C variance.c:300-345)
 *   svtgpu_aom_highbd_10_variance{W}x{H} ≙ svt_aom_highbd_10_variance{W}x{H} (aom_dsp_rtcd.h:544-570, C EbPsnr.c:174-214);
 *       its pointers are CONVERT_TO_BYTEPTR-encoded uint16_t planes, as in the reference (EbDefinitions.h:950-951). */
uint32_t     svtgpu_aom_sad4x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad4x4x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance4x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance4x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad4x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad4x8x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance4x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance4x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad8x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad8x4x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance8x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance8x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad8x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad8x8x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance8x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance8x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad8x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad8x16x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance8x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance8x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad16x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad16x8x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance16x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance16x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad16x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad16x16x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance16x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance16x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad16x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad16x32x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance16x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance16x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad32x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad32x16x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance32x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance32x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad32x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad32x32x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance32x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance32x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad32x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad32x64x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance32x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance32x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad64x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad64x32x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance64x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance64x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad64x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad64x64x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance64x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance64x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad64x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad64x128x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance64x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance64x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad128x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad128x64x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance128x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance128x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad128x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad128x128x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance128x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance128x128(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad4x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad4x16x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance4x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance4x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad16x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad16x4x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance16x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance16x4(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad8x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad8x32x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance8x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance8x32(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad32x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad32x8x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance32x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance32x8(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad16x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad16x64x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance16x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance16x64(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
uint32_t     svtgpu_aom_sad64x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride);
void         svtgpu_aom_sad64x16x4d(const uint8_t *src, int src_stride, const uint8_t *const ref[], int ref_stride, uint32_t *sad_array);
unsigned int svtgpu_aom_variance64x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
unsigned int svtgpu_aom_highbd_10_variance64x16(const uint8_t *src, int src_stride, const uint8_t *ref, int ref_stride, unsigned int *sse);
/* ≙ sad_16b_kernel (aom_dsp_rtcd.h:861, C svt_aom_sad_16b_kernel_c EbComputeSAD_C.c:39) */
uint32_t svtgpu_sad_16b_kernel(uint16_t *src, uint32_t src_stride, uint16_t *ref, uint32_t ref_stride, uint32_t height,
                               uint32_t width);
/* ≙ svt_aom_sse / svt_aom_highbd_sse (aom_dsp_rtcd.h:54-56, C EbEncInterPrediction.c:562-590; highbd takes plain
 * uint16_t planes cast to uint8_t*) */
int64_t svtgpu_aom_sse(const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int width, int height);
int64_t svtgpu_aom_highbd_sse(const uint8_t *a8, int a_stride, const uint8_t *b8, int b_stride, int width, int height);
/* ≙ svt_spatial_full_distortion_kernel / svt_full_distortion_kernel16_bits (common_dsp_rtcd.h:169-171) */
uint64_t svtgpu_spatial_full_distortion_kernel(uint8_t *input, uint32_t input_offset, uint32_t input_stride,
                                               uint8_t *recon, int32_t recon_offset, uint32_t recon_stride,
                                               uint32_t area_width, uint32_t area_height);
uint64_t svtgpu_full_distortion_kernel16_bits(uint8_t *input, uint32_t input_offset, uint32_t input_stride,
                                              uint8_t *recon, int32_t recon_offset, uint32_t recon_stride,
                                              uint32_t area_width, uint32_t area_height);
/* ≙ svt_nxm_sad_kernel / svt_nxm_sad_kernel_sub_sampled (aom_dsp_rtcd.h:853-854): the MD fast-loop N x M SAD
 * (C svt_fast_loop_nxm_sad_kernel, EbComputeSAD_C.c:20; the C "sub-sampled" entry is the full SAD too, :209) */
uint32_t svtgpu_nxm_sad_kernel(const uint8_t *src, uint32_t src_stride, const uint8_t *ref, uint32_t ref_stride,
                               uint32_t height, uint32_t width);
uint32_t svtgpu_nxm_sad_kernel_sub_sampled(const uint8_t *src, uint32_t src_stride, const uint8_t *ref,
                                           uint32_t ref_stride, uint32_t height, uint32_t width);
/* ≙ svt_aom_mse16x16 (aom_dsp_rtcd.h:241, C EbPsnr.c:76) and svt_aom_highbd_8_mse16x16 (:262, C variance.c:453;
 * 16-bit samples CONVERT_TO_BYTEPTR-encoded, *sse only) */
uint32_t svtgpu_aom_mse16x16(const uint8_t *src_ptr, int32_t source_stride, const uint8_t *ref_ptr,
                             int32_t recon_stride, uint32_t *sse);
void     svtgpu_aom_highbd_8_mse16x16(const uint8_t *src_ptr, int32_t source_stride, const uint8_t *ref_ptr,
                                      int32_t recon_stride, uint32_t *sse);
/* ≙ variance_highbd (aom_dsp_rtcd.h:867, C svt_aom_variance_highbd_c variance.c:278): any w x h, 16-bit */
uint32_t svtgpu_aom_variance_highbd(const uint16_t *a, int a_stride, const uint16_t *b, int b_stride, int w, int h,
                                    uint32_t *sse);
/* ≙ svt_aom_sub_pixel_variance{W}x{H} (aom_dsp_rtcd.h:587-753, C SUBPIX_VAR variance.c:308): 2-tap bilinear
 * (1/8 pel offsets xoffset, yoffset in 0..7) of a (H + 1) x (W + 1) source window, then the W x H variance */
uint32_t svtgpu_aom_sub_pixel_variance4x4(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance4x8(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance8x4(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance8x8(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance8x16(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance16x8(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance16x16(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance16x32(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance32x16(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance32x32(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance32x64(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance64x32(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance64x64(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance64x128(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance128x64(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance128x128(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance4x16(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance16x4(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance8x32(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance32x8(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance16x64(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);
uint32_t svtgpu_aom_sub_pixel_variance64x16(const uint8_t *src_ptr, int source_stride, int xoffset, int yoffset, const uint8_t *ref_ptr, int ref_stride, uint32_t *sse);

/* Batched MD distortion (the frame-level GPU boundary; no single reference equivalent: it evaluates what
 * the MD candidate loops evaluate block by block through svt_aom_mefn_ptr, av1me.c:29-174).
 * For every 64x64 SB of `source` and every reference frame r at the SB's full-pel motion vector
 * mv[sb][r] = {x, y}, svtgpu_md_dist_batch computes the raw moments of every 4x4 cell of the SB (moments[sb][r][256],
 * cells in raster order, 8 bytes each: x = SAD | (uint16_t)(signed sum) << 16, y = SSE of the differences): every
 * block of every AV1 shape <= 64x64 tiling the SB has exact sums of its cells' moments.  svtgpu_md_expand derives,
 * for an SB range, every block's
 *   q = 0: SAD (sad{W}x{H} / sad_16b_kernel), q = 1: the *sse the variance function reports,
 *   q = 2: the variance (8-bit: svt_aom_variance{W}x{H}; 10-bit: svt_aom_highbd_10_variance{W}x{H}, which round only
 *          the block totals, EbPsnr.c:183-214);
 * svtgpu_md_read expands and reads an SB range.
 * Samples outside the frame read the nearest edge sample (the encoder's padded pictures).
 * Expanded layout: out[sb][r][q][SVTGPU_MD_BLOCKS]; shapes in BlockSize order without the 128 shapes,
 * blocks of one shape in raster order (svtgpu_md_layout). */
#define SVTGPU_MD_SHAPES 19
#define SVTGPU_MD_BLOCKS 849
typedef struct SvtGpuMdBatch SvtGpuMdBatch;
int     svtgpu_md_batch_create(SvtGpuContext *ctx, int32_t width, int32_t height, int32_t nref, SvtGpuMdBatch **out);
void    svtgpu_md_batch_destroy(SvtGpuMdBatch *b);
int32_t svtgpu_md_batch_nsb(const SvtGpuMdBatch *b);
int     svtgpu_md_set_mvs(SvtGpuMdBatch *b, const int16_t *mv, void *stream); /* host [nsb][nref][2] */
int     svtgpu_md_dist_batch(SvtGpuMdBatch *b, const SvtGpuFrame *source, const SvtGpuFrame *const *refs,
                             int32_t sb_begin, int32_t sb_end, void *stream);
/* every block's values of SBs [sb_begin, sb_end) from the last batch's moments, into the expanded table (in stream
 * order; svtgpu_md_out_device_ptr) -- for a consumer that wants per-shape values rather than the moments */
int     svtgpu_md_expand(SvtGpuMdBatch *b, int32_t sb_begin, int32_t sb_end, void *stream);
/* expands SBs [sb_begin, sb_end) and copies their rows [sb][r][3][SVTGPU_MD_BLOCKS] to `out` (synchronous) */
int     svtgpu_md_read(SvtGpuMdBatch *b, uint32_t *out, int32_t sb_begin, int32_t sb_end, void *stream);
void   *svtgpu_md_out_device_ptr(SvtGpuMdBatch *b);     /* the expanded table [nsb][nref][3][SVTGPU_MD_BLOCKS] */
void   *svtgpu_md_moments_device_ptr(SvtGpuMdBatch *b); /* the cell moments [nsb][nref][256] (uint32 pairs) */
/* shape_w/shape_h/shape_offset: [SVTGPU_MD_SHAPES] block dims and first output index of each shape */
void    svtgpu_md_layout(int32_t *shape_w, int32_t *shape_h, int32_t *shape_offset);


/* =========================================================================================
 * Open-loop motion-estimation SAD
 * ========================================================================================= */
#ifndef SVTGPU_BOOL_T
#define SVTGPU_BOOL_T
typedef uint8_t Bool; /* EbSvtAv1.h:82 */
#endif
/* RTCD-compatible shims (synchronous, host pointers), each replacing the pointer it names:
 * svt_ext_all_sad_calculation_8x8_16x16 (aom_dsp_rtcd.h:850; C EbMotionEstimation.c:336) -- 8 positions x .. x+7 of a
 *   64x64 block: 8x8 / 16x16 SADs (Z-order), best SAD/MV updates (strict <), p_eight_sad16x16[16][8] */
void svtgpu_ext_all_sad_calculation_8x8_16x16(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                              uint32_t mv, uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16,
                                              uint32_t *p_best_mv8x8, uint32_t *p_best_mv16x16,
                                              uint32_t p_eight_sad16x16[16][8], uint32_t p_eight_sad8x8[64][8],
                                              Bool sub_sad);
/* svt_ext_eight_sad_calculation_32x32_64x64 (aom_dsp_rtcd.h:851; C EbMotionEstimation.c:370) */
void svtgpu_ext_eight_sad_calculation_32x32_64x64(uint32_t p_sad16x16[16][8], uint32_t *p_best_sad_32x32,
                                                  uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                                  uint32_t *p_best_mv64x64, uint32_t mv, uint32_t p_sad32x32[4][8]);
/* svt_ext_sad_calculation_8x8_16x16 (aom_dsp_rtcd.h:839; C EbMotionEstimation.c:99) -- one 16x16 at one position */
void svtgpu_ext_sad_calculation_8x8_16x16(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                                          uint32_t *p_best_sad_8x8, uint32_t *p_best_sad_16x16, uint32_t *p_best_mv8x8,
                                          uint32_t *p_best_mv16x16, uint32_t mv, uint32_t *p_sad16x16,
                                          uint32_t *p_sad8x8, Bool sub_sad);
/* svt_ext_sad_calculation_32x32_64x64 (aom_dsp_rtcd.h:845; C EbMotionEstimation.c:172) */
void svtgpu_ext_sad_calculation_32x32_64x64(uint32_t *p_sad16x16, uint32_t *p_best_sad_32x32,
                                            uint32_t *p_best_sad_64x64, uint32_t *p_best_mv32x32,
                                            uint32_t *p_best_mv64x64, uint32_t mv, uint32_t *p_sad32x32);
/* svt_sad_loop_kernel (aom_dsp_rtcd.h:776; C EbComputeSAD_C.c:58) -- full search of a block over an area */
void svtgpu_sad_loop_kernel(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                            uint32_t block_height, uint32_t block_width, uint64_t *best_sad, int16_t *x_search_center,
                            int16_t *y_search_center, uint32_t src_stride_raw, uint8_t skip_search_line,
                            int16_t search_area_width, int16_t search_area_height);
/* svt_pme_sad_loop_kernel (aom_dsp_rtcd.h:866; C EbProductCodingLoop.c:1801) -- the MD full-pel refinement: cost =
 * SAD + svt_aom_fp_mv_err_cost (mcomp.c:771) over the reference's visiting order; mv_cost_params is the reference's
 * MV_COST_PARAMS (mcomp.h:37), read with its layout */
struct svt_mv_cost_param;
void svtgpu_pme_sad_loop_kernel(const struct svt_mv_cost_param *mv_cost_params, uint8_t *src, uint32_t src_stride,
                                uint8_t *ref, uint32_t ref_stride, uint32_t block_height, uint32_t block_width,
                                uint32_t *best_cost, int16_t *best_mvx, int16_t *best_mvy,
                                int16_t search_position_start_x, int16_t search_position_start_y,
                                int16_t search_area_width, int16_t search_area_height, int16_t search_step,
                                int16_t mvx, int16_t mvy);
/* Frame level: the integer full-pel search of every 64x64 block against every reference (≙ the per-block
 * open_loop_me_fullpel_search_sblock, EbMotionEstimation.c:782-818, after the best SADs are reset to MAX_SAD_VALUE,
 * :1363-1364).  origin[sb][r] = {x, y} is the search-area origin relative to the block (the MV of search position
 * (0, 0)); the search covers sa_w x sa_h positions (sa_w <= 192); sub_sad = the SUB_SAD_SEARCH method (8x8 SADs over
 * rows 0, 2, 4, 6, doubled).  8-bit luma; reference samples outside the frame read the nearest edge sample (the
 * padded reference pictures).  Output per (sb, r): 85 best SADs and MVs -- [0, 64) 8x8, [64, 80) 16x16, [80, 84) 32x32,
 * [84] 64x64, in the reference's Z-order numbering (me_ctx->p_best_sad_8x8 ...); MV = (y << 16) | (uint16_t)x. */
#define SVTGPU_ME_BLOCKS 85
typedef struct SvtGpuMeBatch SvtGpuMeBatch;
int  svtgpu_me_batch_create(SvtGpuContext *ctx, int32_t width, int32_t height, int32_t nref, SvtGpuMeBatch **out);
void svtgpu_me_batch_destroy(SvtGpuMeBatch *b);
int  svtgpu_me_set_origins(SvtGpuMeBatch *b, const int16_t *origin, void *stream); /* host [nsb][nref][2] */
int  svtgpu_me_search(SvtGpuMeBatch *b, const SvtGpuFrame *source, const SvtGpuFrame *const *refs, int32_t sa_w,
                      int32_t sa_h, int32_t sub_sad, int32_t sb_begin, int32_t sb_end, void *stream);
int  svtgpu_me_read(SvtGpuMeBatch *b, uint32_t *best_sad, uint32_t *best_mv, int32_t sb_begin, int32_t sb_end,
                    void *stream); /* host [sb_end - sb_begin][nref][85] each (nullable) */

/* =========================================================================================
 * Overlapped-block motion compensation (OBMC) distortion; 8-bit only, as in the reference
 * ========================================================================================= */
/* RTCD-compatible shims (synchronous, host pointers) for the 22 block sizes, installed by svtgpu_install_obmc_rtcd
 * (svtgpu_rtcd.h).  wsrc and mask are compact (stride W); diff = wsrc - pre * mask.
 * ≙ svt_aom_obmc_sad{W}x{H} (aom_dsp_rtcd.h:354-396; C sad_av1.c:18-62): sum of (|diff| + 2048) >> 12 */
unsigned int svtgpu_aom_obmc_sad4x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad4x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad8x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad8x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad8x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad16x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad16x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad16x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad32x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad32x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad32x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad64x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad64x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad64x128(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad128x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad128x128(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad4x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad16x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad8x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad32x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad16x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
unsigned int svtgpu_aom_obmc_sad64x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask);
/* ≙ svt_aom_obmc_variance{W}x{H} (aom_dsp_rtcd.h:398-440; C OBMC_VAR variance.c:347-373): d = diff rounded >> 12 away
 * from zero on ties (ROUND_POWER_OF_TWO_SIGNED); *sse = sum d^2; returns *sse - (sum d)^2 / (W * H) */
unsigned int svtgpu_aom_obmc_variance4x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance4x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance8x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance8x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance8x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance16x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance16x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance16x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance32x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance32x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance32x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance64x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance64x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance64x128(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance128x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance128x128(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance4x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance16x4(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance8x32(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance32x8(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance16x64(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_variance64x16(const uint8_t *pre, int pre_stride, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
/* ≙ svt_aom_obmc_sub_pixel_variance{W}x{H} (aom_dsp_rtcd.h:442-484; C OBMC_SUBPIX_VAR variance.c:375-390): the 2-tap
 * bilinear interpolation (1/8 pel offsets in 0..7) of a (H + 1) x (W + 1) window of pre, then the OBMC variance */
unsigned int svtgpu_aom_obmc_sub_pixel_variance4x4(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance4x8(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance8x4(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance8x8(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance8x16(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance16x8(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance16x16(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance16x32(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance32x16(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance32x32(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance32x64(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance64x32(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance64x64(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance64x128(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance128x64(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance128x128(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance4x16(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance16x4(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance8x32(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance32x8(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance16x64(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);
unsigned int svtgpu_aom_obmc_sub_pixel_variance64x16(const uint8_t *pre, int pre_stride, int xoffset, int yoffset, const int32_t *wsrc, const int32_t *mask, unsigned int *sse);

/* Frame level: the full-pel OBMC refinement of many blocks at once (≙ svt_av1_obmc_full_pixel_search, av1me.c:760-776:
 * obmc_refining_search_sad, :721-758, then the OBMC variance at the MV it ends on).  One item = one call of the
 * reference's function: the start MV is clamped to the limits, best = obmc_sad(start) + cost, and each of up to
 * search_range steps visits the neighbours {-1,0},{0,-1},{0,1},{1,0},{-1,1},{1,1},{1,-1},{-1,-1} ({row, col}; the
 * first four only when search_diag == 0) inside the limits in that order; a neighbour takes over when its SAD is
 * below the running best both before and after its cost is added; the walk stops at a step nobody takes.
 * Reference samples outside the frame read the nearest edge sample (the padded reference pictures, as svtgpu_me_search).
 *
 * Pools (host arrays given to svtgpu_obmc_set_items, copied to the device):
 *   wm_pool    int32: an item's wsrc is wm_pool[wm_offset .. + w*h), its mask wm_pool[wm_offset + w*h .. + 2*w*h),
 *              both compact (stride w); wm_offset is a multiple of 4.
 *   cost_pool  int32, read by cost_mode 1 items only, at cost_offset, with T = 2 * search_range + 1:
 *                [0, 4)          the joint costs x->nmv_vec_cost[MV_JOINT_ZERO, HNZVZ, HZVNZ, HNZVNZ]
 *                [4, 4 + T)      row costs:    entry k = x->mv_cost_stack[0][clip((r0 + k - (ref_mv_row >> 3)) * 8)]
 *                [4 + T, 4 + 2T) column costs: entry k = x->mv_cost_stack[1][clip((c0 + k - (ref_mv_col >> 3)) * 8)]
 *              where r0 / c0 = the start row / column after the clamp to the limits, minus search_range, and clip is
 *              CLIP3(MV_LOW, MV_UPP, .) as in svt_mv_cost (mcomp.h:135).
 * cost_mode 0 = mvsad_err_cost_light (av1me.c:237; approx_inter_rate): 1296 + 50 * 8 * (|dcol| + |drow|) against the
 * centre >> 3, no tables.  cost_mode 1 = mvsad_err_cost (av1me.c:254): ROUND_POWER_OF_TWO((unsigned)(joint + row +
 * column) * sad_per_bit, AV1_PROB_COST_SHIFT).
 *
 * The result's variance is the ovf value alone: the caller adds svt_aom_mv_err_cost (or _light) of the final MV, which
 * needs its RD tables (get_obmc_mvpred_var, av1me.c:709-720). */
#define SVTGPU_OBMC_MAX_RANGE 16
typedef struct SvtGpuObmcItem {
    int32_t ref;                                /* index into refs[] of svtgpu_obmc_search */
    int32_t x, y;                               /* block origin in the frame (luma samples) */
    int32_t w, h;                               /* one of the 22 AV1 block sizes */
    int32_t mvp_col, mvp_row;                   /* mvp_full: the full-pel start MV */
    int32_t ref_mv_col, ref_mv_row;             /* ref_mv: the centre MV in 1/8 pel */
    int32_t col_min, col_max, row_min, row_max; /* x->mv_limits (full pel, within [-16384, 16384]) */
    int32_t sad_per_bit;                        /* sadpb */
    int32_t search_range;                       /* obmc_ctrls.fpel_search_range, <= SVTGPU_OBMC_MAX_RANGE */
    int32_t search_diag;                        /* obmc_ctrls.fpel_search_diag */
    int32_t cost_mode;                          /* 0: approx_inter_rate, 1: the cost tables */
    int32_t wm_offset, cost_offset;             /* into the pools, in int32 entries */
} SvtGpuObmcItem;
typedef struct SvtGpuObmcResult {
    int32_t  mv_col, mv_row; /* dst_mv (full pel) */
    uint32_t best_sad;       /* obmc_refining_search_sad's return: SAD + cost at dst_mv */
    uint32_t variance, sse;  /* ovf at dst_mv and its *sse */
    int32_t  steps;          /* moves the walk made */
} SvtGpuObmcResult;
typedef struct SvtGpuObmcBatch SvtGpuObmcBatch;
int  svtgpu_obmc_batch_create(SvtGpuContext *ctx, int32_t width, int32_t height, int32_t nref, int32_t max_items,
                              SvtGpuObmcBatch **out);
void svtgpu_obmc_batch_destroy(SvtGpuObmcBatch *b);
/* checks every item (SVTGPU_ERR_INVALID_ARG on an unknown size, search_range > 16, ref >= nref, an origin outside
 * the frame, empty or oversized limits, an offset outside its pool: nothing is uploaded and the batch holds no items)
 * and uploads the list and the pools; synchronous */
int  svtgpu_obmc_set_items(SvtGpuObmcBatch *b, const SvtGpuObmcItem *items, int32_t nitems, const int32_t *wm_pool,
                           int32_t wm_count, const int32_t *cost_pool, int32_t cost_count, void *stream);
/* svtgpu_obmc_set_items without the pool upload: checks and uploads the items and the costs as that entry does (the same
 * refusals, but no pool pointer), sizes the batch's device pool to wm_count entries and returns its address in *wm_dev for
 * svtgpu_obmc_weighted_src_batch to fill.  The address holds until a later call asks for a larger pool.  Queue the fill and
 * svtgpu_obmc_search on one stream.  The batch type is declared above this entry's section; SvtGpuObmcBlock further down. */
int svtgpu_obmc_set_items_device_wm(SvtGpuObmcBatch *b, const SvtGpuObmcItem *items, int32_t nitems, int32_t wm_count,
                                    const int32_t *cost_pool, int32_t cost_count, int32_t **wm_dev, void *stream);
/* items [item_begin, item_end) of the current list against refs[nref] (8-bit frames of the batch's size) */
int  svtgpu_obmc_search(SvtGpuObmcBatch *b, const SvtGpuFrame *const *refs, int32_t item_begin, int32_t item_end,
                        void *stream);
int  svtgpu_obmc_read(SvtGpuObmcBatch *b, SvtGpuObmcResult *out, int32_t item_begin, int32_t item_end,
                      void *stream); /* host [item_end - item_begin]; synchronous */

/* =========================================================================================
 * Frame-buffer work around the path
 * ========================================================================================= */
/* RTCD-compatible shims (synchronous, host pointers):
 * svt_convert_8bit_to_16bit / svt_convert_16bit_to_8bit (common_dsp_rtcd.h:154-156; C EbPackUnPack_C.c:270-283) */
void svtgpu_convert_8bit_to_16bit(uint8_t *src, uint32_t src_stride, uint16_t *dst, uint32_t dst_stride, uint32_t width,
                                  uint32_t height);
void svtgpu_convert_16bit_to_8bit(uint16_t *src, uint32_t src_stride, uint8_t *dst, uint32_t dst_stride, uint32_t width,
                                  uint32_t height);
/* svt_aom_generate_padding / svt_aom_generate_padding16_bit (EbMcp.h:46-51; C EbMcp.c:95-240): src_pic is the padded
 * buffer's first sample, the visible area starts at (padding_width, padding_height) */
void svtgpu_aom_generate_padding(uint8_t *src_pic, uint32_t src_stride, uint32_t original_src_width,
                                 uint32_t original_src_height, uint32_t padding_width, uint32_t padding_height);
void svtgpu_aom_generate_padding16_bit(uint16_t *src_pic, uint32_t src_stride, uint32_t original_src_width,
                                       uint32_t original_src_height, uint32_t padding_width, uint32_t padding_height);
/* svt_extend_frame (EbRestoration.c:197): data = first visible sample (CONVERT_TO_BYTEPTR-encoded when highbd) */
void svtgpu_extend_frame(uint8_t *data, int32_t width, int32_t height, int32_t stride, int32_t border_horz,
                         int32_t border_vert, int32_t highbd);
/* Device-pointer versions (asynchronous on `stream`, nullable = the library's default stream); bits = 8 or 16,
 * strides in samples: */
int svtgpu_convert_plane(const void *src, int32_t src_bits, int32_t src_stride, void *dst, int32_t dst_bits,
                         int32_t dst_stride, int32_t width, int32_t height, void *stream);
int svtgpu_pad_plane(void *buf, int32_t bits, int32_t stride, int32_t width, int32_t height, int32_t pad_width,
                     int32_t pad_height, void *stream);
int svtgpu_extend_plane(void *data, int32_t bits, int32_t stride, int32_t width, int32_t height, int32_t border_horz,
                        int32_t border_vert, void *stream);
/* svt_convert_pic_8bit_to_16bit (EbRestProcess.c:235-272) and the 16 -> 8 copy-back of non-reference pictures
 * (EbRestProcess.c:670-697) on device frames: all three planes, direction from the frames' bit depths */
int svtgpu_frame_convert(const SvtGpuFrame *src, SvtGpuFrame *dst, void *stream);

/* =========================================================================================
 * Super-resolution: the normative horizontal upscale between CDEF and loop restoration
 * (svt_av1_superres_upscale_frame, EbRestProcess.c:405-458; svt_av1_upscale_normative_rows, EbSuperRes.c:214-284)
 * ========================================================================================= */
/* calculate_scaled_size_helper (EbSuperRes.c:22-41): the downscaled size of `dim` for a scale denominator.  8 leaves
 * it unchanged, 9..16 give dim * 8 / denom rounded to nearest and at least min(16, dim), 17 is the 3/4 code of the
 * reference's resize mode; any other value returns dim.  Host only. */
int32_t svtgpu_superres_scaled_size(int32_t dim, int32_t denom);
/* The step and the start phase (14 fractional bits) of an upscale of in_w to out_w samples (plane widths):
 * av1_get_upscale_convolve_step / get_upscale_convolve_x0 (EbSuperRes.c:43-52).  Host only. */
int svtgpu_superres_geometry(int32_t in_w, int32_t out_w, int32_t *x_step_qn, int32_t *x0_qn);
/* One plane, device pointers, asynchronous on `stream` (nullable = the library's default stream) like
 * svtgpu_convert_plane; bits = 8 or 16, strides and widths in samples.  Output column X < out_w samples source
 * position x0_qn + X * x_step_qn whatever the picture's tile columns are (the reference carries the phase across
 * them).  Source indices are clamped to [0, src_plane_width - 1]: src_plane_width is the downscaled picture's coded
 * plane width (mi_cols * 4 >> sub_x), where the reference starts replicating, and the columns between in_w and it are
 * read as they lie.  Every column of [0, dst_plane_width) is written: those at and past out_w repeat the row's last
 * upscaled sample.  in_w <= out_w <= 2 * in_w; 16-bit samples are below 1 << 15 (bit_depth 8..12). */
int svtgpu_superres_upscale_plane(const void *src, int32_t bits, int32_t src_stride, int32_t src_plane_width,
                                  int32_t in_w, void *dst, int32_t dst_stride, int32_t dst_plane_width, int32_t out_w,
                                  int32_t rows, int32_t bit_depth, void *stream);
/* svt_av1_superres_upscale_frame: the three planes of `src` (crop width frame_width; the coded width is frame_width
 * rounded up to 8) into `dst` (crop width upscaled_width), chroma widths rounded up, all rows of the frames.
 * SVTGPU_ERR_INVALID_ARG: src == dst, unequal heights or bit depths, frame_width > src's width, upscaled_width >
 * dst's width, upscaled_width < frame_width, or 2 * frame_width < upscaled_width (the denominator cannot exceed 16).
 * Equal widths copy the planes. */
int svtgpu_superres_upscale_frame(const SvtGpuFrame *src, SvtGpuFrame *dst, int32_t frame_width, int32_t upscaled_width,
                                  void *stream);

/* =========================================================================================
 * The non-normative frame resizer (svt_av1_resize_plane / svt_aom_resize_frame, EbResize.c:148-973): the down-scaler of
 * the source picture of a superres or resized frame, of scaled_input_pic before the LR search and of reference pictures
 * at another size, and its up-scaler (the normative table), bit-exact with svt_av1_resize_plane_c /
 * svt_av1_highbd_resize_plane_c and their _horizontal variants
 * ========================================================================================= */
/* The plan of one 1-D resize of in_length to out_length samples (resize_multistep, EbResize.c:353-387): `steps`
 * factor-of-2 halvings (get_down2_steps; each takes a length n to (n + 1) >> 1, by svt_av1_down2_symeven when n is even
 * and down2_symodd when it is odd), then, unless the halved length -- in_length halved `steps` times -- already equals
 * out_length, one svt_av1_interpolate_core of that length: filter_index 0..4 names the table (the 0.5 / 0.625 / 0.75 /
 * 0.875-band down-scaling tables and the normative up-scaling table, choose_interp_filter), delta and offset are its
 * position step and start (14 fractional bits): output x reads taps (y >> 14) - 3 + k, k = 0..7, of phase (y >> 8) & 63
 * at y = offset + 128 + x * delta.  filter_index = -1, delta = offset = 0: no interpolation (equal lengths: a copy).
 * 1 <= lengths <= 65536 and out_length <= 2 * in_length, else SVTGPU_ERR_INVALID_ARG.  Host only. */
int svtgpu_resize_plan(int32_t in_length, int32_t out_length, int32_t *steps, int32_t *filter_index, int32_t *delta,
                       int32_t *offset);
/* The library's tables, for a test to hold them to the reference's: table filter_index (0..4 as above) as [64 phases]
 * [8 taps], and the two half filters of the halvings (svt_aom_av1_down2_symeven_half_filter,
 * av1_down2_symodd_half_filter).  Host only. */
int svtgpu_resize_filter(int32_t filter_index, int16_t out[64][8]);
int svtgpu_resize_half_filters(int16_t symeven[4], int16_t symodd[4]);
/* One plane, device pointers, asynchronous on `stream` (nullable = the library's default stream) like
 * svtgpu_superres_upscale_plane; bits = 8 or 16, strides in samples.  Every row goes from in_w to out_w, rounded and
 * clipped, then every column from in_h to out_h; a direction of equal lengths is copied.  Exactly out_w x out_h
 * samples of dst are written.  SVTGPU_ERR_INVALID_ARG without a launch: a null pointer, overlapping buffers, bits not 8
 * or 16, a width beyond its stride, a non-positive size, a size above 65536, an up-scale beyond 2x in a direction
 * (down-scales of any ratio are accepted), bit_depth outside 8..12 or not 8 for 8-bit samples.
 * Workspace: the intermediate plane and the buffers of multi-step halvings come from one device allocation per stream
 * that the library keeps and grows (a stream synchronise, a free and an allocation, only when a call needs more than
 * every call before it on that stream; nothing is allocated otherwise).  Calls on one stream reuse it in stream order,
 * so any number may be queued back to back; calls on different streams use different workspaces and may overlap; host
 * threads that enqueue on the same stream take turns inside the call.  The workspace of a stream is kept until the
 * process ends: destroy a stream only after its last resize has completed. */
int svtgpu_resize_plane(const void *src, int32_t bits, int32_t src_stride, int32_t in_w, int32_t in_h, void *dst,
                        int32_t dst_stride, int32_t out_w, int32_t out_h, int32_t bit_depth, void *stream);
/* svt_aom_resize_frame (EbResize.c:887-973): the three 4:2:0 planes of `src` (crop size src_w x src_h, at most the
 * frame's size) into `dst` (crop size dst_w x dst_h); chroma sizes are (dim + 1) >> 1 on both sides.  Equal sizes copy
 * the crop.  The samples of dst outside the crop are left as they are: SvtGpuFrame has no border, so the padding the
 * reference ends with (svt_aom_generate_padding) stays with the caller, by svtgpu_pad_plane on its own padded buffers.
 * SVTGPU_ERR_INVALID_ARG before any launch: src == dst, unequal bit depths, a crop size beyond its frame, or a plane
 * that svtgpu_resize_plane would refuse. */
int svtgpu_resize_frame(const SvtGpuFrame *src, SvtGpuFrame *dst, int32_t src_w, int32_t src_h, int32_t dst_w,
                        int32_t dst_h, void *stream);
/* RTCD-compatible shims of svt_av1_resize_plane / svt_av1_highbd_resize_plane (aom_dsp_rtcd.h:898-901): host pointers,
 * synchronous, staged through a device buffer of the calling thread.  0 (EB_ErrorNone), or 0x80001005
 * (EB_ErrorBadParameter) for sizes svtgpu_resize_plane refuses. */
SVTGPU_ERROR_T svtgpu_av1_resize_plane(const uint8_t *const input, int height, int width, int in_stride, uint8_t *output,
                                       int height2, int width2, int out_stride);
SVTGPU_ERROR_T svtgpu_av1_highbd_resize_plane(const uint16_t *const input, int height, int width, int in_stride,
                                              uint16_t *output, int height2, int width2, int out_stride, int bd);

/* =========================================================================================
 * The temporal filter's filter half (EbTemporalFiltering.c): the noise estimate (svt_estimate_noise_fp16_c /
 * svt_estimate_noise_highbd_fp16_c, :3672-3740) and the block loop of produce_temporally_filtered_pic (:2939-3301) from
 * apply_filtering_central to get_final_filtered_pixels, bit-exact with the reference's C.  The motion half -- motion
 * estimation, the sub-pel searches and the inter prediction -- is not in this section (the compensation and the sub-pel
 * search have their own below; HME / ME stays on the host); what it leaves behind is this section's input: the predictor
 * planes of every reference picture and, per (reference, 64x64 block), one SvtGpuTfBlock.
 * ========================================================================================= */
/* What the search left in MeContext for one 64x64 block of one reference (tf_32x32_block_split_flag, tf_32x32_mv_x / _y,
 * tf_16x16_mv_x / _y, tf_32x32_block_error, tf_16x16_block_error); 256 bytes.  Index 4 * idx_32x32 + q is 16x16 quadrant
 * q of 32x32 block idx_32x32 (raster order both). */
typedef struct SvtGpuTfBlock {
    int32_t  split32[4];
    int16_t  mv32_x[4], mv32_y[4];
    int16_t  mv16_x[16], mv16_y[16];
    uint64_t err32[4];
    uint64_t err16[16];
} SvtGpuTfBlock;
/* tf_decay_factor_fp16[3], tf_mv_dist_th, tf_chroma of MeContext, the encoder bit depth (8 or 10: 8-bit or 16-bit
 * samples) and tf_ctrls.use_zz_based_filter */
typedef struct SvtGpuTfParams {
    uint32_t decay_factor_fp16[3];
    int32_t  mv_dist_th;
    int32_t  tf_chroma;
    int32_t  bit_depth;
    int32_t  use_zz_based_filter;
} SvtGpuTfParams;
/* The three 4:2:0 planes of a picture as device pointers to the sample at (0, 0), strides in samples.  Every plane is
 * readable (the output: writable) over the 64-aligned area 64 * ceil(w / 64) x 64 * ceil(h / 64), chroma halved: the
 * reference filters whole 64x64 blocks, and a quadrant's window error at the right or bottom edge covers the picture's
 * padding, which the caller supplies as the reference's padded pictures do.  Pointers are 16-byte aligned and strides a
 * multiple of 16 bytes. */
typedef struct SvtGpuTfPlanes {
    void   *plane[3];
    int32_t stride[3];
} SvtGpuTfPlanes;
typedef struct SvtGpuTfState SvtGpuTfState;
/* The state of one picture size (width and height multiples of 8): the device copy of the metadata and the result slot
 * of the asynchronous noise estimate.  One state serves one picture at a time. */
int  svtgpu_tf_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, SvtGpuTfState **out);
void svtgpu_tf_state_destroy(SvtGpuTfState *state);
/* The noise estimate of a w x h plane (device pointer; bits = 8: uint8_t samples, 10: uint16_t samples of 10 bits; any
 * w, h >= 1): the Sobel gate ga < 50 and |Laplacian| sum over the interior, (sum * 82137) / (6 * num), or -65536 when
 * fewer than 16 samples pass.  Synchronous: *out_fp16 is valid on return. */
int svtgpu_tf_estimate_noise(SvtGpuContext *ctx, const void *plane, int32_t bits, int32_t stride, int32_t w, int32_t h,
                             void *stream, int32_t *out_fp16);
/* The same in stream order with no host wait: the division happens on the device and the value lands in the state;
 * svtgpu_tf_read_noise copies it out (and waits for `stream`). */
int svtgpu_tf_estimate_noise_async(SvtGpuTfState *state, const void *plane, int32_t bits, int32_t stride, int32_t w,
                                   int32_t h, void *stream);
int svtgpu_tf_read_noise(SvtGpuTfState *state, void *stream, int32_t *out_fp16);
/* One picture: `centre` filtered with n_refs predictor pictures `refs[n_refs]` into `out` (out may be centre: every
 * workgroup reads its block before it writes it).  blocks[r * nblk + b] is reference r, block b in raster order, nblk =
 * ceil(w / 64) * ceil(h / 64); host memory, copied before the call returns.  The caller leaves out the references that
 * the reference's outlier and brightness tests skip (:3008-3032) and the centre itself.  Whole 64x64 blocks are written.
 * With tf_chroma == 0 the chroma planes of out are the centre's.  Runs in stream order with no host wait (the call waits
 * only for the previous call's metadata upload on this state).  SVTGPU_ERR_UNSUPPORTED: n_refs > 26 (the reference's
 * 16-bit count holds 27 contributions of at most 1000).  SVTGPU_ERR_INVALID_ARG before any launch: a null pointer,
 * n_refs < 0, a bit depth other than 8 or 10, a plane that is misaligned or narrower than the aligned width. */
int svtgpu_tf_filter_frame(SvtGpuTfState *state, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs, int32_t n_refs,
                           const SvtGpuTfBlock *blocks, const SvtGpuTfParams *params, const SvtGpuTfPlanes *out,
                           void *stream);
/* Host-only bookkeeping.  svt_aom_noise_log1p_fp16 (:656-675); and tf_decay_factor_fp16 of one plane from its
 * decay_control, the log1p of its noise level and q (:2913-2937: q_decay_fp8 = q * q >> 5 from q = 128 up, else
 * max(q << 2, 1); n_decay_fp10 = decay_control * (0.7 + noise_log1p) / 64).  The caller derives q and decay_control. */
int32_t  svtgpu_tf_noise_log1p_fp16(int32_t noise_level_fp16);
uint32_t svtgpu_tf_decay_factor_fp16(int32_t decay_control, int32_t noise_log1p_fp16, int32_t q);
/* The library's log1p_tab_fp16, sqrt_array_fp16 [16] and expf_tab_fp16, for a test to hold them to the reference's. */
int svtgpu_tf_tables(const int32_t **log1p_fp16, int32_t *n_log1p, const uint32_t **sqrt_fp16, const int32_t **expf_fp16,
                     int32_t *n_expf);
/* RTCD shims: host pointers, synchronous, staged through a device buffer of the calling thread.  The two noise
 * functions carry the reference's prototypes (aom_dsp_rtcd.h:874-877).  The other seven pointers take struct MeContext *
 * (and EbPictureBufferDesc *), whose layouts this library does not know: svtgpu_rtcd.h's adapters, compiled inside the
 * encoder, read the fields and call these (idx_32x32 = tf_block_col + 2 * tf_block_row; params' bit_depth and
 * use_zz_based_filter are not read: the entry names both).  accum / count are indexed with the predictor's stride, as
 * in the reference. */
int32_t svtgpu_estimate_noise_fp16(const uint8_t *src, uint16_t width, uint16_t height, uint16_t stride_y);
int32_t svtgpu_estimate_noise_highbd_fp16(const uint16_t *src, int width, int height, int stride, int bd);
void svtgpu_tf_apply_planewise_medium(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                      const uint8_t *y_src, int y_src_stride, const uint8_t *y_pre, int y_pre_stride,
                                      const uint8_t *u_src, const uint8_t *v_src, int uv_src_stride, const uint8_t *u_pre,
                                      const uint8_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                      unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum, uint16_t *y_count,
                                      uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count);
void svtgpu_tf_apply_planewise_medium_hbd(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                          const uint16_t *y_src, int y_src_stride, const uint16_t *y_pre, int y_pre_stride,
                                          const uint16_t *u_src, const uint16_t *v_src, int uv_src_stride,
                                          const uint16_t *u_pre, const uint16_t *v_pre, int uv_pre_stride,
                                          unsigned int block_width, unsigned int block_height, int ss_x, int ss_y,
                                          uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count,
                                          uint32_t *v_accum, uint16_t *v_count, uint32_t encoder_bit_depth);
void svtgpu_tf_apply_zz_planewise_medium(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                         const uint8_t *y_pre, int y_pre_stride, const uint8_t *u_pre, const uint8_t *v_pre,
                                         int uv_pre_stride, unsigned int block_width, unsigned int block_height, int ss_x,
                                         int ss_y, uint32_t *y_accum, uint16_t *y_count, uint32_t *u_accum,
                                         uint16_t *u_count, uint32_t *v_accum, uint16_t *v_count);
void svtgpu_tf_apply_zz_planewise_medium_hbd(const SvtGpuTfBlock *blk, int32_t idx_32x32, const SvtGpuTfParams *prm,
                                             const uint16_t *y_pre, int y_pre_stride, const uint16_t *u_pre,
                                             const uint16_t *v_pre, int uv_pre_stride, unsigned int block_width,
                                             unsigned int block_height, int ss_x, int ss_y, uint32_t *y_accum,
                                             uint16_t *y_count, uint32_t *u_accum, uint16_t *u_count, uint32_t *v_accum,
                                             uint16_t *v_count, uint32_t encoder_bit_depth);
void svtgpu_tf_apply_filtering_central(int32_t tf_chroma, int32_t src_stride_y, uint8_t **src, uint32_t **accum,
                                       uint16_t **count, uint16_t blk_width, uint16_t blk_height, uint32_t ss_x,
                                       uint32_t ss_y);
void svtgpu_tf_apply_filtering_central_highbd(int32_t tf_chroma, int32_t src_stride_y, uint16_t **src_16bit,
                                              uint32_t **accum, uint16_t **count, uint16_t blk_width, uint16_t blk_height,
                                              uint32_t ss_x, uint32_t ss_y);
void svtgpu_tf_get_final_filtered_pixels(int32_t tf_chroma, uint8_t **src_center_ptr_start,
                                         uint16_t **altref_buffer_highbd_start, uint32_t **accum, uint16_t **count,
                                         const uint32_t *stride, int blk_y_src_offset, int blk_ch_src_offset,
                                         uint16_t blk_width_ch, uint16_t blk_height_ch, int is_highbd);

/* =========================================================================================
 * AV1 sub-pel interpolation (single reference) and the temporal filter's motion compensation.  The per-block family
 * svt_av1_convolve_{2d,x,y,2d_copy}_sr and svt_av1_highbd_convolve_*_sr (EbInterPrediction.c:320-427, :679-786: what the
 * reference's svt_aom_convolve[][][0] / svt_aom_convolveHbd[][][0] tables hold), and tf_64x64_inter_prediction /
 * tf_32x32_inter_prediction (EbTemporalFiltering.c:2230-2580) for every (reference, 64x64 block) of a picture in one launch,
 * bit-exact with the reference's C.  With it the device chain of the temporal filter is: upload the padded reference
 * pictures, svtgpu_tf_predict_frame, svtgpu_tf_filter_frame; the host supplies the per-block motion records only.  The
 * tf_*_sub_pel_search walks are the next section's, the compound (jnt_) convolves the one after and the masked compounds the
 * one after that; ME / HME, the scaled convolves and intrabc stay on the host.
 * ========================================================================================= */
/* RTCD shims: host pointers, synchronous, staged through a device buffer of the calling thread.  filter_x / filter_y are
 * the 8-tap kernel rows already selected for the phase (av1_get_interp_filter_subpel_kernel of the InterpFilterParams);
 * round_0 / round_1 are the ConvolveParams' (get_conv_params_no_round: 3 / 11, at 12 bits 5 / 9).  The four forms read
 * what the reference's C reads: 2d both rows, rows -3 .. h + 3 and columns -3 .. w + 4 of src; x filter_x and round_0,
 * columns -3 .. w + 4; y filter_y, rows -3 .. h + 4; copy neither.  w, h in {2, 4, 8, 16, 32, 64, 128}; bd 8 for the
 * 8-bit entries, 10 or 12 for the highbd ones.  svtgpu_rtcd.h's adapters carry the reference's prototypes. */
void svtgpu_av1_convolve_2d_sr(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                               int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                               int32_t round_1);
void svtgpu_av1_convolve_x_sr(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                              int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                              int32_t round_1);
void svtgpu_av1_convolve_y_sr(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                              int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                              int32_t round_1);
void svtgpu_av1_convolve_2d_copy_sr(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                                    int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                                    int32_t round_1);
void svtgpu_av1_highbd_convolve_2d_sr(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                      int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                      int32_t round_0, int32_t round_1, int32_t bd);
void svtgpu_av1_highbd_convolve_x_sr(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                     int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                     int32_t round_0, int32_t round_1, int32_t bd);
void svtgpu_av1_highbd_convolve_y_sr(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                     int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                     int32_t round_0, int32_t round_1, int32_t bd);
void svtgpu_av1_highbd_convolve_2d_copy_sr(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                           int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                           int32_t round_0, int32_t round_1, int32_t bd);
/* The library's six filter tables, [6][16][8] int16: sub_pel_filters_8, _8smooth, _8sharp, bilinear_filters,
 * sub_pel_filters_4, sub_pel_filters_4smooth, for a test to hold them to the reference's. */
int svtgpu_interp_tables(const int16_t **tables, int32_t *n_tables);
/* What the temporal filter's search left in MeContext for one (reference, 64x64 block), as far as the compensation reads
 * it; 368 bytes.  use64: the block took the tf_64x64_inter_prediction path (tf_64x64_mv_x / _y) and nothing else is read.
 * split32[i]: tf_32x32_block_split_flag; split16[4 * i + j]: tf_16x16_block_split_flag[i][j]; mv32 / mv16 / mv8:
 * tf_32x32_mv, tf_16x16_mv [4 * i + j], tf_8x8_mv [16 * i + 4 * j + k] (i, j, k raster indices of the 32x32 block in the
 * 64x64, the 16x16 in the 32x32, the 8x8 in the 16x16).  MVs are in 1/8 luma sample. */
typedef struct SvtGpuTfMotion {
    int16_t mv64_x, mv64_y;
    uint8_t use64, reserved0[3];
    uint8_t split32[4];
    uint8_t split16[16];
    uint8_t reserved1[4];
    int16_t mv32_x[4], mv32_y[4];
    int16_t mv16_x[16], mv16_y[16];
    int16_t mv8_x[64], mv8_y[64];
} SvtGpuTfMotion;
/* The motion compensation of one picture: for every reference r and 64x64 block b, the predictor of the block from
 * refs[r] with motion[r * nblk + b] (host memory, copied before the call returns) into pred[r], in exactly the layout
 * svtgpu_tf_filter_frame reads: whole 64x64 blocks over the 64-aligned area, pred planes 16-byte aligned with strides a
 * multiple of 16 bytes.  The 8-tap sharp filter (4-tap for the 4x4 chroma of an 8x8 block), MV clamp and phase as
 * compute_subpel_params / clamp_mv_to_umv_border_sb with the edges tf_*_inter_prediction builds.  refs[r].plane[p] points
 * at sample (0, 0) of the padded reference picture; border_x / border_y (luma samples, chroma halved) is the padding that
 * is readable around the state's width x height on every side, and strides are at least width + 2 * border_x.  Every read
 * coordinate is clamped into [-border, size + border - 1], so no MV makes the kernel read outside the planes; from a
 * border of 72 the clamp never acts (a clamped MV reaches 64 + 4 + 3 samples out) and the result is the reference's.
 * tf_chroma == 0 leaves the chroma predictors untouched: plane[1] / plane[2] of refs and pred are then neither checked nor
 * read and may be null.  Runs in stream order with no host wait, the state's metadata
 * buffer reused as by svtgpu_tf_filter_frame.  SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any
 * launch: a null pointer, n_refs < 0, a bit depth other than 8 or 10, a negative border, a misaligned or too narrow plane. */
int svtgpu_tf_predict_frame(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                            int32_t border_y, const SvtGpuTfMotion *motion, int32_t bit_depth, int32_t tf_chroma,
                            const SvtGpuTfPlanes *pred, void *stream);

/* =========================================================================================
 * The temporal filter's sub-pel motion search: the `frame_index != index_center` section of
 * produce_temporally_filtered_pic (EbTemporalFiltering.c:3087-3261) for every (reference, 64x64 block) of a picture in one
 * launch -- tf_64x64 / 32x32 / 16x16 / 8x8_sub_pel_search (svt_check_position, tf_subpel_search, :1535-2228), the
 * 64-vs-32 test, the pred_error_32x32_th bypass and derive_tf_32x32_block_split_flag (:240-289) -- bit-exact with the
 * reference's C.  It leaves one SvtGpuTfMotion and one SvtGpuTfBlock per (reference, block) in a device buffer of the
 * state, which svtgpu_tf_compensate_filter_frame consumes in stream order: search -> compensation -> filter without the
 * records leaving the device.  Only HME / ME (svt_aom_motion_estimation_b64, full-pel) stays on the host.
 * ========================================================================================= */
/* What full-pel ME left for one (reference, 64x64 block): p_best_mv64x64[0], p_best_mv32x32, p_best_mv16x16, p_best_mv8x8
 * as (x, y) in whole samples, in SvtGpuTfMotion's nested raster indices (the caller's adapter applies tab16x16 / tab8x8);
 * every component within [-2047, 2047] (its eighth-sample form and the 7/8 the walk adds then fit the reference's int16).
 * force64: the host's `tf_use_pred_64x64_only_th && (th == 0xFF || tf_use_64x64_pred())`; with th == 0xFF the caller
 * puts hme_sc_x / _y into mv64.  352 bytes. */
typedef struct SvtGpuTfFullpel {
    int16_t mv64_x, mv64_y;
    int16_t mv32_x[4], mv32_y[4];
    int16_t mv16_x[16], mv16_y[16];
    int16_t mv8_x[64], mv8_y[64];
    uint8_t force64, reserved[11];
} SvtGpuTfFullpel;
/* tf_ctrls as the search reads them: the three pel modes (0 off, 1 all eight positions, 2 no diagonals), use_2tap (64x64
 * and 32x32 take BILINEAR, else EIGHTTAP_REGULAR; 16x16 and 8x8 always regular), sub_sampling_shift (0 or 1),
 * enable_8x8_pred, subpel_early_exit_th (0 .. 255), the bit depth of the planes searched (8 or 10; with use_8bit_subpel a
 * 10-bit encode passes its 8-bit planes and 8) and pred_error_32x32_th. */
typedef struct SvtGpuTfSearchParams {
    int32_t  half_pel_mode, quarter_pel_mode, eight_pel_mode;
    int32_t  use_2tap;
    int32_t  sub_sampling_shift;
    int32_t  enable_8x8_pred;
    int32_t  subpel_early_exit_th;
    int32_t  bit_depth;
    uint64_t pred_error_32x32_th;
} SvtGpuTfSearchParams;
/* The search of one picture: luma only.  centre: as svtgpu_tf_filter_frame's (readable over the 64-aligned area, 16-byte
 * aligned, stride a multiple of 16 bytes); refs[r].plane[0]: sample (0, 0) of the padded reference picture with border_x /
 * border_y readable samples around it, as svtgpu_tf_predict_frame's (every read coordinate is clamped into the border; from
 * a border of 72 the clamp never acts).  fullpel[r * nblk + b]: host memory, copied before the call returns.  A field of
 * the records that neither the compensation nor the filter reads under the block's flags is 0: under use64 everything but
 * use64, mv64 and the block record's mv32 (= mv64, which the filter reads) -- err32 of such a block is not a search result
 * and is written by svtgpu_tf_compensate_filter_frame; of an unsplit 32x32 block mv16 / mv8 / split16 / err16; of a split
 * one mv32 / err32, and mv16 (motion record) or mv8 by split16.  Runs in stream order with no host wait.
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch: a null pointer, n_refs < 0, a bit depth
 * other than 8 or 10, a mode outside 0 .. 2, another parameter out of range, a full-pel MV beyond 2047, a negative border,
 * a misaligned or too narrow plane. */
int svtgpu_tf_search_frame(SvtGpuTfState *state, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs, int32_t n_refs,
                           int32_t border_x, int32_t border_y, const SvtGpuTfFullpel *fullpel,
                           const SvtGpuTfSearchParams *params, void *stream);
/* Copies the records of the last search (n_refs as searched) to host memory and waits for `stream`. */
int svtgpu_tf_search_read(SvtGpuTfState *state, int32_t n_refs, SvtGpuTfMotion *motion_out, SvtGpuTfBlock *blocks_out,
                          void *stream);
/* The rest of the chain on the state's records: svtgpu_tf_predict_frame's kernel on the motion records (refs, borders and
 * pred as there; bit depth and tf_chroma are filter_params'), then err32 of every use64 block from the predictor against
 * the centre (convert_64x64_info_to_32x32_info, :2665-2733: the variance of each 32x32 quadrant over 32 >> sub_sampling_shift
 * rows at doubled strides, shifted back), then svtgpu_tf_filter_frame's kernel on the block records into `out`.  No record
 * is uploaded and the host does not wait.  n_refs is the last search's.  Refusals as the two sibling entries'. */
int svtgpu_tf_compensate_filter_frame(SvtGpuTfState *state, const SvtGpuTfPlanes *centre, const SvtGpuTfPlanes *refs,
                                      int32_t n_refs, int32_t border_x, int32_t border_y,
                                      const SvtGpuTfParams *filter_params, int32_t sub_sampling_shift,
                                      const SvtGpuTfPlanes *pred, const SvtGpuTfPlanes *out, void *stream);

/* =========================================================================================
 * AV1 compound (two-reference) inter prediction.  The per-block family svt_av1_jnt_convolve_{2d,x,y,2d_copy} and
 * svt_av1_highbd_jnt_convolve_* (EbInterPrediction.c:503-677, :861-1040: what the reference's svt_aom_convolve[][][1] /
 * svt_aom_convolveHbd[][][1] tables hold), the frame-distance weights of COMPOUND_DISTWTD
 * (svt_av1_dist_wtd_comp_weight_assign, :276-318), and svt_aom_inter_prediction (EbEncInterPrediction.c:4070) with
 * is_compound = 1 for a list of blocks in one launch, bit-exact with the reference's C.  The masked compounds
 * (COMPOUND_WEDGE, COMPOUND_DIFFWTD) are the next section's; scaled references (warped motion, OBMC blending and inter-intra: their own sections),
 * intrabc and 12-bit pictures at frame level (the shims handle 12 bits) stay on the host.
 * ========================================================================================= */
/* RTCD shims: host pointers, synchronous, staged through a device buffer of the calling thread.  filter_x / filter_y are
 * the 8-tap kernel rows already selected for the phase, as for the _sr shims; the other arguments are the ConvolveParams
 * spelt out: round_0 / round_1 (get_conv_params_no_round with is_compound = 1: 3 / 7, at 12 bits 5 / 7; each 0 .. 7),
 * conv_dst / conv_dst_stride (its dst: CONV_BUF_TYPE, stride in elements >= w), do_average, use_jnt_comp_avg, fwd_offset,
 * bck_offset.  do_average == 0 writes only conv_dst -- the rounded sum with its 1 << offset_bits bias -- and leaves dst
 * alone (dst may be null); do_average == 1 reads conv_dst, combines by (tmp + res) >> 1 or, with use_jnt_comp_avg, by
 * (tmp * fwd_offset + res * bck_offset) >> 4, removes the two offsets, rounds by 14 - round_0 - round_1 and clips to the bit
 * depth into dst; conv_dst is then left as it was.  Each form reads of src what its C function reads (as the _sr shims).
 * w, h in {4, 8, 16, 32, 64, 128}; bd 8 for the 8-bit entries, 10 or 12 for the highbd ones.  svtgpu_rtcd.h's adapters carry
 * the reference's prototypes. */
void svtgpu_av1_jnt_convolve_2d(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                                int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                                int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average,
                                int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset);
void svtgpu_av1_jnt_convolve_x(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                               int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                               int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average,
                               int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset);
void svtgpu_av1_jnt_convolve_y(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                               int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                               int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average,
                               int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset);
void svtgpu_av1_jnt_convolve_2d_copy(const uint8_t *src, int32_t src_stride, uint8_t *dst, int32_t dst_stride, int32_t w,
                                     int32_t h, const int16_t *filter_x, const int16_t *filter_y, int32_t round_0,
                                     int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average,
                                     int32_t use_jnt_comp_avg, int32_t fwd_offset, int32_t bck_offset);
void svtgpu_av1_highbd_jnt_convolve_2d(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                       int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                       int32_t round_0, int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride,
                                       int32_t do_average, int32_t use_jnt_comp_avg, int32_t fwd_offset,
                                       int32_t bck_offset, int32_t bd);
void svtgpu_av1_highbd_jnt_convolve_x(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                      int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                      int32_t round_0, int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride,
                                      int32_t do_average, int32_t use_jnt_comp_avg, int32_t fwd_offset,
                                      int32_t bck_offset, int32_t bd);
void svtgpu_av1_highbd_jnt_convolve_y(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                      int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                      int32_t round_0, int32_t round_1, uint16_t *conv_dst, int32_t conv_dst_stride,
                                      int32_t do_average, int32_t use_jnt_comp_avg, int32_t fwd_offset,
                                      int32_t bck_offset, int32_t bd);
void svtgpu_av1_highbd_jnt_convolve_2d_copy(const uint16_t *src, int32_t src_stride, uint16_t *dst, int32_t dst_stride,
                                            int32_t w, int32_t h, const int16_t *filter_x, const int16_t *filter_y,
                                            int32_t round_0, int32_t round_1, uint16_t *conv_dst,
                                            int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg,
                                            int32_t fwd_offset, int32_t bck_offset, int32_t bd);
/* The two offsets of COMPOUND_DISTWTD from the frame distances: d0 = |distance from the current frame to the forward
 * reference|, d1 = |distance to the backward reference| (clamped to MAX_FRAME_DISTANCE = 31 here, as the reference clamps
 * them), order_idx 0 or 1; the table walk of svt_av1_dist_wtd_comp_weight_assign.  The offsets sum to 16.  Host only.
 * SVTGPU_ERR_INVALID_ARG: a negative distance, an order_idx outside 0 / 1, a null pointer. */
int svtgpu_dist_wtd_weights(int32_t d0, int32_t d1, int32_t order_idx, int32_t *fwd_offset, int32_t *bck_offset);
typedef struct SvtGpuCompoundBlock {      /* one bi-predicted block; 32 bytes */
    int16_t x, y;                          /* luma position of the block in the picture, multiples of 4 */
    uint8_t w_log2, h_log2;                /* luma size 8 .. 128; min(w, h) >= 8 (is_comp_ref_allowed), ratio <= 4 */
    uint8_t ref0, ref1;                    /* indices into refs[] */
    int16_t mv0_x, mv0_y, mv1_x, mv1_y;    /* 1/8 luma sample */
    uint8_t filter_x, filter_y;            /* 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR (dual filter) */
    uint8_t dist_wtd;                      /* 0 COMPOUND_AVERAGE, 1 COMPOUND_DISTWTD with the two offsets below */
    uint8_t fwd_offset, bck_offset;        /* as svtgpu_dist_wtd_weights; ignored when dist_wtd == 0 */
    uint8_t reserved[11];
} SvtGpuCompoundBlock;
/* The bi-predicted blocks of one picture in one launch: for every block of blocks[n_blocks] (host memory, copied before
 * the call returns) the compound predictor from refs[ref0] with (mv0_x, mv0_y) and refs[ref1] with (mv1_x, mv1_y) into
 * `pred` at the block's position, luma and -- with chroma != 0 -- the two 4:2:0 chroma planes; what svt_aom_inter_prediction
 * writes with is_compound = 1, COMPOUND_AVERAGE or COMPOUND_DISTWTD, translation, unscaled references, no OBMC and no
 * inter-intra: its MV clamp (clamp_mv_to_umv_border_sb with the block's own edges), position and phase arithmetic, the
 * chroma block at ((x >> 3) << 3) / 2, per direction the 4-tap tables when that dimension of the plane's block is <= 4
 * (av1_get_convolve_filter_params), per plane and reference the copy / x / y / 2-D form by which phases are non-zero.
 * The sizes are the seventeen AV1 block sizes from 8x8 to 128x128 (128 only beside 64 or 128).  Samples of pred outside
 * the listed blocks are left alone; blocks that overlap give an unspecified one of their results.
 * `state` gives the picture size (width and height multiples of 8: the area a block must stay inside) and the grow-only
 * metadata buffer, as for svtgpu_tf_predict_frame; refs[r].plane[p] points at sample (0, 0) of a padded reference picture
 * with border_x / border_y (luma samples, chroma halved) readable samples on every side and strides of at least width +
 * 2 * border_x; pred->plane[p] at sample (0, 0) of the predictor picture, 16-byte aligned with strides of at least the
 * width and a multiple of 16 bytes.  Every read coordinate is clamped into [-border, size + border - 1], so no MV makes
 * the kernel read outside the planes; a clamped MV reaches the block's size + 4 + 3 samples out of the plane, so from a
 * border of the largest listed block's luma size + 14 (142 for 128x128: its 64-wide chroma reaches 71 chroma samples)
 * the clamp never acts and the result is the reference's.  On edge-replicated borders it is the reference's from any
 * border.  chroma == 0 leaves planes 1 and 2 unread and unwritten (they may be null).  Bit depth 8 or 10.  Runs in stream
 * order with no host wait (the call waits only for the previous call's metadata upload on this state).
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch: a null pointer, n_refs < 0, n_blocks < 0,
 * a bit depth other than 8 or 10, a negative border, a misaligned or too narrow plane, a block that leaves the picture
 * area or is not at a multiple of 4, a size outside the rule, a ref index >= n_refs, a filter kind above 3, dist_wtd above
 * 1, offsets that do not sum to 16 when dist_wtd is set.  n_blocks == 0 returns 0 and launches nothing. */
int svtgpu_compound_predict_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                  int32_t border_y, const SvtGpuCompoundBlock *blocks, int32_t n_blocks, int32_t bit_depth,
                                  int32_t chroma, const SvtGpuTfPlanes *pred, void *stream);

/* =========================================================================================
 * AV1 masked compound inter prediction: COMPOUND_WEDGE and COMPOUND_DIFFWTD, the other two of the four inter-inter
 * compound types.  The DIFFWTD mask svt_av1_build_compound_diffwtd_mask_d16 (C_DEFAULT/EbInterPrediction_c.c:15-40), the
 * blends svt_aom_lowbd_blend_a64_d16_mask / svt_aom_highbd_blend_a64_d16_mask (EbBlend_a64_mask.c:34-195), the wedge masks
 * of svt_av1_init_wedge_masks (EbInterPrediction.c:1445-2132), and svt_aom_inter_prediction with a masked compound type
 * (reference 1 through av1_make_masked_scaled_inter_predictor, EbEncInterPrediction.c:50-164) for a list of blocks,
 * bit-exact with the reference's C.  Inter-intra (it needs intra prediction), warped and scaled
 * references, the encoder's wedge / DIFFWTD search (pick_wedge, svt_av1_wedge_sse_from_residuals) and 12-bit pictures at
 * frame level stay on the host.
 * ========================================================================================= */
/* RTCD shims: host pointers, synchronous, staged through a device buffer of the calling thread; the ConvolveParams spelt
 * out as round_0 / round_1 (each 0 .. 7, their sum at most 14).  w, h in {4, 8, 16, 32, 64, 128}; strides in elements.
 * The mask shim writes mask[h][w] packed with stride w, as the reference does: m = min(38 + (|src0 - src1| rounded by
 * 14 - round_0 - round_1 + bd - 8) / 16, 64), or 64 - m for mask_type 1 (DIFFWTD_38_INV); bd 8, 10 or 12.  The blend shims
 * write dst = clip(round(((m * src0 + (64 - m) * src1) >> 6) - the two offsets, 14 - round_0 - round_1)) with m the mask
 * value (subw = subh = 0), the rounded mean of a 2x2 (1, 1), or AOM_BLEND_AVG of a horizontal (1, 0) or vertical (0, 1)
 * pair; they read (h << subh) rows of (w << subw) mask bytes, mask_stride >= w << subw.  src0 / src1 may alias dst (all
 * reads happen first).  bd 8 for the lowbd entry; 8, 10 or 12 for the highbd one, whose dst is the uint16_t block behind a
 * uint8_t pointer, as in the reference.  svtgpu_rtcd.h's adapters carry the reference's prototypes. */
void svtgpu_av1_build_compound_diffwtd_mask_d16(uint8_t *mask, int32_t mask_type, const uint16_t *src0, int32_t src0_stride,
                                                const uint16_t *src1, int32_t src1_stride, int32_t h, int32_t w,
                                                int32_t round_0, int32_t round_1, int32_t bd);
void svtgpu_aom_lowbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                         const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask,
                                         uint32_t mask_stride, int32_t w, int32_t h, int32_t subw, int32_t subh,
                                         int32_t round_0, int32_t round_1);
void svtgpu_aom_highbd_blend_a64_d16_mask(uint8_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                          const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask,
                                          uint32_t mask_stride, int32_t w, int32_t h, int32_t subw, int32_t subh,
                                          int32_t round_0, int32_t round_1, int32_t bd);
/* The wedge mask svt_aom_get_contiguous_soft_mask(wedge_index, wedge_sign, bsize) of a w x h block into mask[h][w], stride
 * w (csrc/wedge_masks.h).  Host only.  SVTGPU_ERR_INVALID_ARG: a size without wedges (they exist for 8x8, 8x16, 16x8, 16x16,
 * 16x32, 32x16, 32x32, 8x32, 32x8), an index outside 0 .. 15, a sign outside 0 / 1, a null pointer. */
int svtgpu_wedge_mask(int32_t w, int32_t h, int32_t wedge_index, int32_t wedge_sign, uint8_t *mask);
typedef struct SvtGpuMaskedCompoundBlock { /* one masked bi-predicted block; 32 bytes; the first 18 as SvtGpuCompoundBlock */
    int16_t x, y;                          /* luma position of the block in the picture, multiples of 4 */
    uint8_t w_log2, h_log2;                /* luma size 8 .. 128; min(w, h) >= 8, ratio <= 4; wedge: 8 .. 32 each way */
    uint8_t ref0, ref1;                    /* indices into refs[] */
    int16_t mv0_x, mv0_y, mv1_x, mv1_y;    /* 1/8 luma sample */
    uint8_t filter_x, filter_y;            /* 0 EIGHTTAP_REGULAR, 1 EIGHTTAP_SMOOTH, 2 MULTITAP_SHARP, 3 BILINEAR (dual filter) */
    uint8_t comp_type;                     /* 0 COMPOUND_WEDGE, 1 COMPOUND_DIFFWTD */
    uint8_t wedge_index, wedge_sign;       /* 0 .. 15, 0 / 1; checked for both types, used by COMPOUND_WEDGE */
    uint8_t mask_type;                     /* 0 DIFFWTD_38, 1 DIFFWTD_38_INV; checked for both types, used by COMPOUND_DIFFWTD */
    uint8_t reserved[10];                  /* must be zero */
} SvtGpuMaskedCompoundBlock;
/* The masked bi-predicted blocks of one picture: for every block of blocks[n_blocks] (host memory, copied before the call
 * returns) the predictor from refs[ref0] with (mv0_x, mv0_y) and refs[ref1] with (mv1_x, mv1_y), blended per sample by the
 * block's wedge mask or by the DIFFWTD mask made from the two luma predictions, into `pred` at the block's position, luma
 * and -- with chroma != 0 -- the two 4:2:0 chroma planes, whose mask values are the rounded means of the luma mask's 2x2s;
 * what svt_aom_inter_prediction writes with is_compound = 1 and COMPOUND_WEDGE or COMPOUND_DIFFWTD, translation, unscaled
 * references, no OBMC and no inter-intra.  Everything svtgpu_compound_predict_batch documents holds here word for word:
 * the MV clamp, position and phase arithmetic, the chroma block at ((x >> 3) << 3) / 2, the 4-tap tables for a dimension
 * <= 4, the form per plane and reference, the seventeen sizes, `state`, refs, pred, the readable border and the read clamp
 * (from a border of the largest listed block's luma size + 14 the result is the reference's; on edge-replicated borders
 * from any border), chroma == 0, bit depth 8 or 10, samples outside the listed blocks left alone, overlapping blocks
 * unspecified.  Runs in stream order with no host wait: one launch, and a second one behind it in the same stream for the
 * chroma of the DIFFWTD blocks, which reads the masks their luma left in a plane of `state` (width x height bytes,
 * allocated at the first such call).  Calls on one state must therefore be queued on one stream, or ordered by the caller.
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch: every refusal of
 * svtgpu_compound_predict_batch that does not concern dist_wtd, and comp_type above 1, a wedge block whose size has no
 * wedges, wedge_index above 15, wedge_sign above 1, mask_type above 1, a non-zero reserved byte.  n_blocks == 0 returns 0
 * and launches nothing. */
int svtgpu_masked_compound_predict_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                         int32_t border_y, const SvtGpuMaskedCompoundBlock *blocks, int32_t n_blocks,
                                         int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream);

/* =========================================================================================
 * AV1 warped-motion (affine) inter prediction: svt_av1_warp_affine / svt_av1_highbd_warp_affine (EbWarpedMotion.c:570, :822),
 * the shear parameters of svt_get_shear_params (:1082-1105), and svt_aom_warped_motion_prediction
 * (EbEncInterPrediction.c:2747) for a list of blocks, bit-exact with the reference's C.  What stays on the host: finding the
 * model (svt_find_projection, svt_aom_select_samples, the global motion search), the chroma of blocks below 16 in a
 * dimension (chroma_plane_warped_motion_prediction_sub8x8, a translation), masked compounds over warped predictors
 * (av1_make_masked_warp_inter_predictor), inter-intra, scaled references, and 12-bit pictures at frame level.
 * ========================================================================================= */
/* svt_get_shear_params on the six model values wmmat (as svt_warp_plane passes them): 1 and abgd = {alpha, beta, gamma,
 * delta} when the model is valid (wmmat[2] > 0) and 4 |alpha| + 7 |beta| < 65536, 4 |gamma| + 4 |delta| < 65536; 0
 * otherwise.  Host only.  SVTGPU_ERR_INVALID_ARG: a null pointer. */
int svtgpu_warp_shear_params(const int32_t wmmat[6], int16_t abgd[4]);
/* The library's warped filter table (the AV1 specification's Warped_Filters): *table points at int16_t[*rows][8], rows = 193,
 * static storage.  Host only.  SVTGPU_ERR_INVALID_ARG: a null pointer. */
int svtgpu_warp_filter_table(const int16_t **table, int32_t *rows);
/* RTCD shims: host pointers, synchronous, staged through a device buffer of the calling thread; the ConvolveParams spelt
 * out: round_0, round_1, is_compound, conv_dst / conv_dst_stride (ConvolveParams::dst, ::dst_stride), do_average,
 * use_jnt_comp_avg, fwd_offset, bck_offset.  Every other argument is the reference's.  The three output modes are the C's:
 * is_compound == 0 writes pred = clip(round(sum, 14 - reduce_bits_horiz) - (1 << (bd - 1)) - (1 << bd)); is_compound with
 * do_average == 0 writes only conv_dst (pred is not looked at and may be null); is_compound with do_average == 1 reads
 * conv_dst, combines by (tmp + sum) >> 1 or, with use_jnt_comp_avg, (tmp * fwd_offset + sum * bck_offset) >> 4, removes the
 * two offsets, rounds by 14 - round_0 - round_1, clips into pred and leaves conv_dst as it was.  Every read of the reference
 * plane is clamped to [0, height - 1] x [0, width - 1].  The highbd form keeps the split reference of this encoder: sample =
 * (ref8b << 2) | ((ref2b >> 6) & 3), two strides; bd 10 or 12; reduce_bits_horiz = round_0 + max(bd + 7 - round_0 - 14, 0).
 * Unlike the other shims these return a code: 0, or SVTGPU_ERR_INVALID_ARG with nothing launched and nothing written for a
 * p_width or p_height that is not a multiple of 8 from 8 to 128 (the AVX2 forms assume the same and every encoder call
 * satisfies it), a null pointer that the mode reads or writes, a stride below its width, subsampling outside 0 / 1, a bd
 * the entry does not take, rounds outside 0 .. 7 or summing above 14, do_average without is_compound, shear parameters
 * outside the two limits above (the filter table has no row for them), or a model whose projection of a unit's centre
 * leaves int32 (undefined in the C).  svtgpu_rtcd.h's adapters carry the reference's prototypes and abort on a refusal. */
int svtgpu_av1_warp_affine(const int32_t *mat, const uint8_t *ref, int32_t width, int32_t height, int32_t stride, uint8_t *pred,
                           int32_t p_col, int32_t p_row, int32_t p_width, int32_t p_height, int32_t p_stride,
                           int32_t subsampling_x, int32_t subsampling_y, int32_t round_0, int32_t round_1, int32_t is_compound,
                           uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg,
                           int32_t fwd_offset, int32_t bck_offset, int16_t alpha, int16_t beta, int16_t gamma, int16_t delta);
int svtgpu_av1_highbd_warp_affine(const int32_t *mat, const uint8_t *ref8b, const uint8_t *ref2b, int32_t width, int32_t height,
                                  int32_t stride8b, int32_t stride2b, uint16_t *pred, int32_t p_col, int32_t p_row,
                                  int32_t p_width, int32_t p_height, int32_t p_stride, int32_t subsampling_x,
                                  int32_t subsampling_y, int32_t bd, int32_t round_0, int32_t round_1, int32_t is_compound,
                                  uint16_t *conv_dst, int32_t conv_dst_stride, int32_t do_average, int32_t use_jnt_comp_avg,
                                  int32_t fwd_offset, int32_t bck_offset, int16_t alpha, int16_t beta, int16_t gamma,
                                  int16_t delta);
typedef struct SvtGpuWarpBlock {          /* one warped block; 64 bytes */
    int16_t x, y;                          /* luma position, multiples of 8 */
    uint8_t w_log2, h_log2;                /* luma size 8 .. 128, min(w, h) >= 8, an AV1 block size */
    uint8_t ref0, ref1;                    /* indices into refs[]; ref1 == 0xFF: one reference */
    uint8_t dist_wtd, fwd_offset, bck_offset, reserved0;   /* as SvtGpuCompoundBlock; ignored with one reference */
    int32_t wmmat0[6], wmmat1[6];          /* as svt_warp_plane passes them (ROTZOOM: [5] = [2], [4] = -[3] set by the caller) */
    uint8_t reserved[4];
} SvtGpuWarpBlock;
/* The warped blocks of one picture in one launch: for every block of blocks[n_blocks] (host memory, copied before the call
 * returns) what svt_aom_warped_motion_prediction writes with no masked compound: the luma of every block, warped from
 * refs[ref0] by wmmat0 -- and, with ref1 != 0xFF, from refs[ref1] by wmmat1, the two averaged or distance-weighted as in
 * svtgpu_compound_predict_batch -- and, with chroma != 0, the two 4:2:0 chroma planes (subsampling_x = subsampling_y = 1, the
 * block at (x / 2, y / 2)) of the blocks with w >= 16 and h >= 16.  A smaller block gets LUMA ONLY: its chroma is a
 * translation in the reference (chroma_plane_warped_motion_prediction_sub8x8) and is not part of this call.  `state`, the
 * plane formats, the pred alignment rules, stream order, n_blocks == 0 and overlapping blocks are
 * svtgpu_compound_predict_batch's, word for word.  There is no border argument: the warp clamps every read row to
 * [0, height - 1] and every column to [0, width - 1] of the reference plane (chroma: the halved dimensions), so
 * refs[r].plane[p] points at sample (0, 0) of a plane with a stride of at least the plane's width and nothing outside the
 * visible picture is read.  The host computes alpha, beta, gamma, delta per reference (svtgpu_warp_shear_params).
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch: a null pointer, n_refs < 0, n_blocks < 0, a
 * bit depth other than 8 or 10, a misaligned or too narrow plane, a block that leaves the picture area or is not at a
 * multiple of 8, a size outside the rule, ref0 >= n_refs, a ref1 that is neither 0xFF nor below n_refs, with two references
 * dist_wtd above 1 or offsets that do not sum to 16 when it is set, a model that svtgpu_warp_shear_params does not return 1
 * for, a model for which wmmat[2] * x + wmmat[3] * y + wmmat[0] (or the other row), evaluated in 64 bits at the centres of
 * the block's corner units, leaves int32. */
int svtgpu_warp_predict_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, const SvtGpuWarpBlock *blocks,
                              int32_t n_blocks, int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream);

/* =========================================================================================
 * AV1 OBMC (overlapped block motion compensation) prediction: the neighbour predictors of build_prediction_by_{above,left}_preds
 * and the blend of av1_build_obmc_inter_prediction (EbEncInterPrediction.c:1144-1590) behind svt_aom_inter_prediction with
 * motion_mode = OBMC_CAUSAL, for a list of single-reference blocks, bit-exact with the reference's C; 8- and 10-bit, 4:2:0,
 * translation, unscaled references.  With empty neighbour lists it is the general single-reference batch predictor (the
 * eight convolve_*_sr forms).  With them: the six per-block blends svt_aom_(highbd_)blend_a64_{v,h}mask as RTCD shims, and the
 * weighted source and mask of svt_aom_precompute_obmc_data (calc_target_weighted_pred, :1767-1827) written on the device into
 * the pool that svtgpu_obmc_search reads.  What stays on the host: the mode-info walk that finds the neighbours
 * (foreach_overlappable_nb_*), the hbd_md weighted sources (10-bit strips unpacked to 8), an
 * svt_av1_calc_target_weighted_pred_* RTCD adapter, OBMC over scaled references, inter-intra over an OBMC prediction (plain
 * inter-intra: the next section) and 12-bit pictures at frame level.
 * ========================================================================================= */
/* RTCD shims of svt_aom_blend_a64_vmask / _hmask (EbBlend_a64_mask.c:302, :350), svt_aom_highbd_blend_a64_vmask_16bit / _hmask_16bit
 * (C_DEFAULT/EbBlend_a64_mask_c.c:15, EbInterPrediction.c:2383) and the two _8bit forms (the same arithmetic on 16-bit samples behind
 * a uint8_t * that is cast back, not shifted, as this encoder's C does): dst = (m * src0 + (64 - m) * src1 + 32) >> 6 with m = mask[row] (vmask) or mask[column] (hmask).
 * Host pointers, synchronous, staged through the calling thread's buffer with one reservation.  w, h powers of two from 1 to
 * 128; strides in elements, at least w; the mask has h (v) or w (h) bytes in 0 .. 64; bd 8, 10 or 12 (not otherwise used).
 * src0 / src1 may alias dst: every read happens before any write.  Bad arguments are fatal, as for the other void shims. */
void svtgpu_aom_blend_a64_vmask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1,
                                uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h);
void svtgpu_aom_blend_a64_hmask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1,
                                uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h);
void svtgpu_aom_highbd_blend_a64_vmask_16bit(uint16_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                             const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h,
                                             int32_t bd);
void svtgpu_aom_highbd_blend_a64_hmask_16bit(uint16_t *dst, uint32_t dst_stride, const uint16_t *src0, uint32_t src0_stride,
                                             const uint16_t *src1, uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h,
                                             int32_t bd);
void svtgpu_aom_highbd_blend_a64_vmask_8bit(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                            const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h,
                                            int32_t bd);
void svtgpu_aom_highbd_blend_a64_hmask_8bit(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                            const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, int32_t w, int32_t h,
                                            int32_t bd);
/* svt_av1_get_obmc_mask: *mask points at the `length` weights of the block's own prediction, static storage; length 1, 2,
 * 4, 8, 16 or 32.  Host only.  SVTGPU_ERR_INVALID_ARG: any other length, a null pointer. */
int svtgpu_obmc_mask(int32_t length, const uint8_t **mask);
typedef struct SvtGpuObmcNeighbour {      /* one overlappable neighbour span; 8 bytes */
    uint8_t rel, size;                     /* offset along the shared edge and length, in units of 4 luma samples */
    uint8_t ref;                           /* index into refs[]: the neighbour's ref_frame[0] */
    uint8_t filters;                       /* filter_x | filter_y << 4, kinds as SvtGpuCompoundBlock */
    int16_t mv_x, mv_y;                    /* the neighbour's mv[0], 1/8 luma sample */
} SvtGpuObmcNeighbour;
typedef struct SvtGpuObmcBlock {          /* one single-reference block with its neighbour lists; 96 bytes */
    int16_t x, y;                          /* luma position, multiples of 8 */
    uint8_t w_log2, h_log2;                /* luma size 8 .. 128, one of the seventeen sizes of SvtGpuCompoundBlock */
    uint8_t ref, filter_x, filter_y;       /* the block's own reference (index into refs[]) and dual filter */
    uint8_t n_above, n_left, reserved0;    /* spans in nb[0 .. n_above) and nb[4 .. 4 + n_left) */
    int16_t mv_x, mv_y;                    /* the block's own MV, 1/8 luma sample */
    int32_t wm_offset;                     /* svtgpu_obmc_weighted_src_batch: where the block's wsrc / mask go; ignored by predict */
    uint8_t reserved[12];                  /* must be zero */
    SvtGpuObmcNeighbour nb[8];             /* above: nb[0 .. n_above); left: nb[4 .. 4 + n_left) */
} SvtGpuObmcBlock;
/* The OBMC_CAUSAL blocks of one picture in one launch: for every block of blocks[n_blocks] (host memory, copied before the
 * call returns) what svt_aom_inter_prediction writes with is_compound = 0, motion_mode = OBMC_CAUSAL and
 * use_precomputed_obmc = 0, luma and -- with chroma != 0 -- the two 4:2:0 chroma planes at (x / 2, y / 2): the block's own
 * prediction from refs[ref] (the convolve_*_sr form by which phases are non-zero, its MV clamp, the 4-tap tables where a
 * dimension of the plane's block is <= 4), blended by the vertical OBMC masks with the predictions of the above spans and
 * then by the horizontal masks with those of the left spans, each blend AOM_BLEND_A64 with its own rounding; the corner
 * takes both, above first.  A span's prediction uses the neighbour's reference, MV and filter kinds at the block's own
 * position; its 4-tap choice and MV clamp are those of the strip the reference predicts (along the edge the span, across it
 * clamp(side >> (ss + 1), 4, 64 >> (ss + 1)) samples of the plane), of which only the blended (min(side, 64) >> 1) >> ss
 * rows or columns are computed.  The chroma of a block whose chroma plane is 4x4, 8x4 or 4x8 takes no above blend
 * (svt_av1_skip_u4x4_pred_in_obmc).  The caller walks its mode-info grid as foreach_overlappable_nb_above / _left do and
 * lists what the walk visited: rel and size of each span (a pair of 4-wide neighbours is one span of size 2 with the
 * second one's motion; a neighbour wider than the block has size = the block's; at most 64 luma samples per span), a compound
 * neighbour with its first reference.  Columns or rows under no listed span keep the block's own prediction.
 * n_above = n_left = 0 is the plain single-reference predictor of the block.
 * `state`, refs, pred, the border and the read clamp, chroma == 0, stream order, n_blocks == 0 and overlapping blocks are
 * svtgpu_compound_predict_batch's, word for word.
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch, pred untouched: a null pointer, n_refs < 0,
 * n_blocks < 0, a bit depth other than 8 or 10, a negative border, a misaligned or too narrow plane, a block that leaves the
 * picture area or is not at a multiple of 8, a size outside the rule, a ref index (the block's or a span's) >= n_refs, a
 * filter kind above 3, a non-zero reserved byte, a neighbour list that is not: sizes powers of two from 2 to 16, rel even,
 * spans ascending without overlap, rel + size <= side / 4, at most max_neighbor_obmc = {1, 2, 3, 4, 4} spans for a side of
 * {8, 16, 32, 64, 128}, no above list at y == 0 and no left list at x == 0. */
int svtgpu_obmc_predict_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                              int32_t border_y, const SvtGpuObmcBlock *blocks, int32_t n_blocks, int32_t bit_depth,
                              int32_t chroma, const SvtGpuTfPlanes *pred, void *stream);

/* wsrc and mask of calc_target_weighted_pred for every block of blocks[n_blocks], 8-bit luma, on the device: wsrc to
 * wm_dev[wm_offset .. + w * h) and mask to wm_dev[wm_offset + w * h .. + 2 * w * h), compact rows of w, the layout
 * svtgpu_obmc_search reads through SvtGpuObmcItem::wm_offset.  Start from wsrc = 0, mask = 64; under every above span, over the
 * blended rows, wsrc = (64 - m) * P and mask = m; both times 64; under every left span, over the blended columns, wsrc =
 * (wsrc >> 6) * m + (P << 6) * (64 - m) and mask = (mask >> 6) * m; finally wsrc = src * 4096 - wsrc.  P are the neighbour
 * luma strips of svtgpu_obmc_predict_batch; the block's own ref, mv and filters are not looked at.  src_luma: an 8-bit device
 * plane at sample (0, 0) of the source picture, src_stride >= width.  wm_dev: device memory, 16-byte aligned, wm_count entries
 * (svtgpu_obmc_set_items_device_wm hands one out).  All seventeen sizes, 8 bits only, like the OBMC distortion family; the
 * hbd_md path stays on the host.  state, refs, border, stream order and n_blocks == 0 as svtgpu_obmc_predict_batch.
 * SVTGPU_ERR_INVALID_ARG before any launch: that entry's refusals that do not concern the block's own ref and filters or pred,
 * a null src_luma or wm_dev, a src_stride below the width, a wm_offset that is negative, no multiple of 4, or whose 2 * w * h
 * entries leave wm_count. */
int svtgpu_obmc_weighted_src_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                   int32_t border_y, const void *src_luma, int32_t src_stride, const SvtGpuObmcBlock *blocks,
                                   int32_t n_blocks, int32_t *wm_dev, int32_t wm_count, void *stream);

/* =========================================================================================
 * AV1 inter-intra prediction: inter_intra_prediction (EbEncInterPrediction.c:2548-2745) behind svt_aom_inter_prediction with
 * is_interintra_used = 1, for a list of single-reference blocks, bit-exact with the reference's C; 8- and 10-bit, 4:2:0,
 * translation, unscaled references.  One launch does the block's single-reference prediction, the intra prediction of the
 * four inter-intra modes (II_DC_PRED, II_V_PRED, II_H_PRED, II_SMOOTH_PRED: build_intra_predictors' edge preparation and the
 * dc / dc_top / dc_left / dc_128 / v / h / smooth predictors), the smooth or wedge mask and the blend
 * (svt_aom_combine_interintra(_highbd), EbInterPrediction.c:2190, :2350).  Beside it: the four-mode luma distortion that
 * inter_intra_search (EbModeDecision.c:275-478) runs per candidate, the smooth masks on the host, and RTCD shims of
 * svt_aom_(highbd_)blend_a64_mask and of the intra predictors.  What stays on the host: reading the recon neighbour arrays
 * and the availability from mode info (the caller hands the raw neighbour samples and counts over), the wedge inter-intra
 * search (pick_interintra_wedge, pick_wedge_fixed_sign, svt_av1_wedge_sse_from_residuals), model_rd_for_sb_with_curvfit,
 * every other intra mode, inter-intra over warped or OBMC predictions or scaled references, and 12-bit pictures at frame level.
 * ========================================================================================= */
#define SVTGPU_II_DC_PRED 0
#define SVTGPU_II_V_PRED 1
#define SVTGPU_II_H_PRED 2
#define SVTGPU_II_SMOOTH_PRED 3
/* build_smooth_interintra_mask (EbInterPrediction.c:2153-2188): the w * h bytes (stride w) of the smooth inter-intra mask of
 * `mode` (0 .. 3, InterIntraMode) for one of the ten plane sizes inter-intra reaches: 4x4, 4x8, 8x4, 8x8, 8x16, 16x8, 16x16,
 * 16x32, 32x16, 32x32.  Host only; the counterpart of svtgpu_wedge_mask and svtgpu_obmc_mask.  SVTGPU_ERR_INVALID_ARG: any
 * other size, a mode above 3, a null pointer. */
int svtgpu_interintra_smooth_mask(int32_t w, int32_t h, int32_t mode, uint8_t *mask);
typedef struct SvtGpuInterIntraBlock {    /* one single-reference inter-intra block; 32 bytes */
    int16_t x, y;                          /* luma position, multiples of 8 */
    uint8_t w_log2, h_log2;                /* luma size, one of 8x8, 8x16, 16x8, 16x16, 16x32, 32x16, 32x32 */
    uint8_t ref, filter_x, filter_y;       /* the reference (index into refs[]) and dual filter, as SvtGpuObmcBlock */
    uint8_t mode;                          /* InterIntraMode: SVTGPU_II_DC_PRED .. SVTGPU_II_SMOOTH_PRED */
    uint8_t use_wedge, wedge_index;        /* 0: the smooth mask of `mode`; 1: wedge `wedge_index` (0 .. 15), sign 0 */
    int16_t mv_x, mv_y;                    /* the MV, 1/8 luma sample */
    uint8_t n_top[2], n_left[2];           /* n_top_px / n_left_px of build_intra_predictors, [0] luma, [1] chroma: 0 .. the
                                              plane's width / height */
    int32_t edge_offset;                   /* where the block's neighbour samples begin in the edge pool */
    uint8_t reserved[8];                   /* must be zero */
} SvtGpuInterIntraBlock;
/* The inter-intra blocks of one picture in one launch: for every block of blocks[n_blocks] (host memory, copied before the
 * call returns) what svt_aom_inter_prediction writes with is_compound = 0, SIMPLE_TRANSLATION and is_interintra_used = 1, luma
 * and -- with chroma != 0 -- the two 4:2:0 chroma planes at (x / 2, y / 2): per plane the block's own prediction from
 * refs[ref] (as svtgpu_obmc_predict_batch with empty lists), blended sample by sample with the intra prediction of
 * interintra_to_intra_mode[mode] at the plane's block size: pred = (m * intra + (64 - m) * inter + 32) >> 6.  m is the smooth
 * mask of (mode, the plane's size), or with use_wedge the wedge mask of the luma size, index wedge_index, sign 0, read for
 * chroma as the rounded mean of its 2x2 luma entries.
 * edges: the edge pool, host memory of n_edges samples of the picture's sample type (uint8_t at 8 bits, uint16_t at 10), copied
 * with the metadata before the call returns.  At edge_offset a block holds above[w], left[h] of luma, then above[w / 2],
 * left[h / 2] of Cb and the same of Cr: the raw neighbour samples, of which above[0 .. n_top) and left[0 .. n_left) are read.
 * The library prepares the edges as build_intra_predictors does for these modes: the last read sample repeated to the side's
 * length; with no samples the other side's first one, or 128 << (bd - 8) less one (above) / plus one (left) when there are
 * none at all; DC takes dc, dc_top, dc_left or dc_128 by which counts are non-zero.  With chroma == 0 the chroma parts need not
 * exist.  A block lies whole inside the state's picture and its MV is clamped against that picture (a block the encoder lets
 * hang over the coded picture's edge is given with its shortened counts; its MV must not need the clamp of the shorter
 * picture).  `state`, refs, pred, the border and the read clamp, stream order, n_blocks == 0 and overlapping blocks are
 * svtgpu_compound_predict_batch's, word for word.
 * SVTGPU_ERR_UNSUPPORTED: n_refs > 26.  SVTGPU_ERR_INVALID_ARG before any launch, pred untouched: a null pointer (edges only
 * when n_blocks > 0), n_refs < 0, n_blocks < 0, n_edges < 0, a bit depth other than 8 or 10, a negative border, a misaligned or
 * too narrow plane, a block that leaves the picture area or is not at a multiple of 8, a size outside the seven, ref >=
 * n_refs, a filter kind above 3, mode > 3, use_wedge > 1, wedge_index > 15, a count above the plane's side, an edge_offset that
 * is negative or whose samples leave n_edges, a non-zero reserved byte. */
int svtgpu_interintra_predict_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                    int32_t border_y, const SvtGpuInterIntraBlock *blocks, int32_t n_blocks, const void *edges,
                                    int32_t n_edges, int32_t bit_depth, int32_t chroma, const SvtGpuTfPlanes *pred, void *stream);
/* inter_intra_search's distortion: for every block i and each mode m = 0 .. 3, luma only, sse_dev[4 * i + m] = the sum of
 * squared differences (svt_aom_sse / svt_aom_highbd_sse) between the source block and the smooth blend
 * (svt_aom_combine_interintra with use_wedge = 0) of the block's inter prediction with mode m's intra prediction.  The blocks'
 * mode, use_wedge and wedge_index are not looked at, nor the chroma counts and edges.  src_luma: a device plane of the
 * picture's sample type at sample (0, 0) of the source, src_stride >= width, in samples.  sse_dev: device memory of 4 *
 * n_blocks int64, 8-byte aligned, written in stream order.  The rest as svtgpu_interintra_predict_batch.
 * SVTGPU_ERR_INVALID_ARG before any launch: that entry's refusals that do not concern pred, mode, use_wedge, wedge_index or
 * chroma; a null src_luma or sse_dev, a misaligned one, a src_stride below the width. */
int svtgpu_interintra_mode_sse_batch(SvtGpuTfState *state, const SvtGpuTfPlanes *refs, int32_t n_refs, int32_t border_x,
                                     int32_t border_y, const SvtGpuInterIntraBlock *blocks, int32_t n_blocks, const void *edges,
                                     int32_t n_edges, int32_t bit_depth, const void *src_luma, int32_t src_stride,
                                     int64_t *sse_dev, void *stream);
/* RTCD shims of svt_aom_blend_a64_mask and svt_aom_highbd_blend_a64_mask (EbBlend_a64_mask.c:201-299): dst = (m * src0 +
 * (64 - m) * src1 + 32) >> 6 with m the mask entry (subw = subh = 0), the rounded mean of the 2x2 entries (1, 1), or the
 * rounded mean of the horizontal (1, 0) or vertical (0, 1) pair.  The high-bit-depth form takes 16-bit samples behind a
 * uint8_t * that is cast, not shifted, as this encoder's C reads them.  Host pointers, synchronous, staged through the calling
 * thread's buffer with one reservation.  w, h powers of two from 1 to 128; strides in elements, at least w; mask_stride at
 * least w << subw; mask entries 0 .. 64; bd 8, 10 or 12 (not otherwise used).  src0 / src1 may alias dst: every read happens
 * before any write.  Bad arguments are fatal, as for the other void shims. */
void svtgpu_aom_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride, const uint8_t *src1,
                               uint32_t src1_stride, const uint8_t *mask, uint32_t mask_stride, int w, int h, int subw, int subh);
void svtgpu_aom_highbd_blend_a64_mask(uint8_t *dst, uint32_t dst_stride, const uint8_t *src0, uint32_t src0_stride,
                                      const uint8_t *src1, uint32_t src1_stride, const uint8_t *mask, uint32_t mask_stride, int w,
                                      int h, int subw, int subh, int bd);
/* The intra predictors inter-intra uses, as two generic entries: the w x h block into dst (stride in samples) from above[w] and
 * left[h], by `kind`: svt_aom_(highbd_)dc / dc_top / dc_left / dc_128 / v / h / smooth _predictor_WxH
 * (EbIntraPrediction.c:1041-1134, :1240+, :1351+).  w, h in {4, 8, 16, 32}; bd 8, 10 or 12.  Host pointers, synchronous; bad
 * arguments are fatal.  svtgpu_install_interintra_rtcd binds the per-size RTCD names to wrappers of these. */
#define SVTGPU_INTRA_DC 0
#define SVTGPU_INTRA_DC_TOP 1
#define SVTGPU_INTRA_DC_LEFT 2
#define SVTGPU_INTRA_DC_128 3
#define SVTGPU_INTRA_V 4
#define SVTGPU_INTRA_H 5
#define SVTGPU_INTRA_SMOOTH 6
void svtgpu_aom_intra_predictor(uint8_t *dst, ptrdiff_t stride, const uint8_t *above, const uint8_t *left, int32_t w, int32_t h,
                                int32_t kind);
void svtgpu_aom_highbd_intra_predictor(uint16_t *dst, ptrdiff_t stride, const uint16_t *above, const uint16_t *left, int32_t w,
                                       int32_t h, int32_t kind, int32_t bd);

/* =========================================================================================
 * Loop restoration
 * ========================================================================================= */
/* RTCD-compatible per-block shims (common_dsp_rtcd.h:174-185).  The Wiener convolve reads round_0 / round_1 of
 * the ConvolveParams (full layout at the top of this header); 16-bit planes are passed CONVERT_TO_BYTEPTR-encoded
 * (EbDefinitions.h:950-951), as in the reference. */
/* ≙ svt_av1_wiener_convolve_add_src (C convolve.c:109-151): 8-tap separable, src row/col -3..+4 */
void svtgpu_av1_wiener_convolve_add_src(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst, ptrdiff_t dst_stride,
                                        const int16_t *filter_x, const int16_t *filter_y, int32_t w, int32_t h,
                                        const SVTGPU_CONVOLVE_PARAMS_T *conv_params);
/* ≙ svt_av1_highbd_wiener_convolve_add_src (C convolve.c:194-232) */
void svtgpu_av1_highbd_wiener_convolve_add_src(const uint8_t *src, ptrdiff_t src_stride, uint8_t *dst,
                                               ptrdiff_t dst_stride, const int16_t *filter_x,
                                               const int16_t *filter_y, int32_t w, int32_t h,
                                               const SVTGPU_CONVOLVE_PARAMS_T *conv_params, int32_t bd);
/* ≙ svt_av1_selfguided_restoration (C EbRestoration.c:923-955): flt0/flt1 of one processing unit, input read
 * with a 3-sample border */
void svtgpu_av1_selfguided_restoration(const uint8_t *dgd8, int32_t width, int32_t height, int32_t dgd_stride,
                                       int32_t *flt0, int32_t *flt1, int32_t flt_stride, int32_t sgr_params_idx,
                                       int32_t bit_depth, int32_t highbd);
/* ≙ svt_apply_selfguided_restoration (C EbRestoration.c:957-991) */
void svtgpu_apply_selfguided_restoration(const uint8_t *dat8, int32_t width, int32_t height, int32_t stride,
                                         int32_t eps, const int32_t *xqd, uint8_t *dst8, int32_t dst_stride,
                                         int32_t *tmpbuf, int32_t bit_depth, int32_t highbd);
/* ≙ svt_av1_compute_stats / _highbd (aom_dsp_rtcd.h:66-68, C EbRestorationPick.c:671 / :708): the Wiener
 * statistics M[win^2] and H[win^2][win^2] of a unit; dgd read with a win/2 border */
void svtgpu_av1_compute_stats(int32_t wiener_win, const uint8_t *dgd8, const uint8_t *src8, int32_t h_start,
                              int32_t h_end, int32_t v_start, int32_t v_end, int32_t dgd_stride, int32_t src_stride,
                              int64_t *M, int64_t *H);
void svtgpu_av1_compute_stats_highbd(int32_t wiener_win, const uint8_t *dgd8, const uint8_t *src8, int32_t h_start,
                                     int32_t h_end, int32_t v_start, int32_t v_end, int32_t dgd_stride,
                                     int32_t src_stride, int64_t *M, int64_t *H, SVTGPU_BIT_DEPTH_T bit_depth);
/* ≙ svt_av1_lowbd_pixel_proj_error / svt_av1_highbd_pixel_proj_error (aom_dsp_rtcd.h:79-81, C :167 / :232) */
int64_t svtgpu_av1_lowbd_pixel_proj_error(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride,
                                          const uint8_t *dat8, int32_t dat_stride, int32_t *flt0, int32_t flt0_stride,
                                          int32_t *flt1, int32_t flt1_stride, int32_t xq[2],
                                          const SVTGPU_SGR_PARAMS_T *params);
int64_t svtgpu_av1_highbd_pixel_proj_error(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride,
                                           const uint8_t *dat8, int32_t dat_stride, int32_t *flt0, int32_t flt0_stride,
                                           int32_t *flt1, int32_t flt1_stride, int32_t xq[2],
                                           const SVTGPU_SGR_PARAMS_T *params);
/* ≙ svt_get_proj_subspace (aom_dsp_rtcd.h:212, C EbRestorationPick.c:560): least-squares xq of a unit */
void svtgpu_get_proj_subspace(const uint8_t *src8, int width, int height, int src_stride, const uint8_t *dat8,
                              int dat_stride, int use_highbitdepth, int32_t *flt0, int flt0_stride, int32_t *flt1,
                              int flt1_stride, int *xq, const SVTGPU_SGR_PARAMS_T *params);

/* Per restoration unit parameters (RestorationUnitInfo, EbRestoration.h:169-188). */
#define SVTGPU_RESTORE_NONE 0
#define SVTGPU_RESTORE_WIENER 1
#define SVTGPU_RESTORE_SGRPROJ 2
typedef struct SvtGpuRestUnit {
    int32_t type;       /* SVTGPU_RESTORE_* */
    int16_t vfilter[8]; /* WienerInfo */
    int16_t hfilter[8];
    int32_t ep;         /* SgrprojInfo */
    int32_t xqd[2];
} SvtGpuRestUnit;

typedef struct SvtGpuLrState SvtGpuLrState;
/* unit_size[plane]: restoration_unit_size (64/128/256 luma; chroma usually luma >> 1).  width / height: the
 * picture's crop size (frm_size.frame_width / _height, EbPictureControlSet.c:1207; any size >= 8), which the
 * restoration units, the search and the filter cover (chroma (width + 1) >> 1, the reference's crop_widths); the
 * frames handed to the search and the apply are the 8-aligned coded size (the deblocking / CDEF extent, mi_cols x 4).
 * Samples right of / below the crop keep the CDEF output in the apply. */
int  svtgpu_lr_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, const int32_t unit_size[3],
                            SvtGpuLrState **out);
void svtgpu_lr_state_destroy(SvtGpuLrState *s);
/* number of units of a plane: horz/vert units (count_units_in_tile, EbRestoration.c:122-124) */
int  svtgpu_lr_units(const SvtGpuLrState *s, int32_t plane, int32_t *hunits, int32_t *vunits);
int  svtgpu_lr_set_units(SvtGpuLrState *s, int32_t plane, const SvtGpuRestUnit *units, void *stream);
/* ≙ svt_av1_loop_restoration_filter_frame(rst_tmpbuf, frame, cm, 0) (EbRestoration.c:1179-1255) with the
 * stripe boundary lines of svt_av1_loop_restoration_save_boundary_lines (EbRestoration.c:1682): rows above /
 * below each 64-row processing stripe come from `deblocked` (the DLF output) inside the frame and from
 * `cdef_out` at the frame top/bottom.  Writes every sample of `out` (planes whose frame_type is NONE are
 * copied).  frame_type[plane]: SVTGPU_RESTORE_NONE or any other value (= per-unit types apply); frame_type == NULL:
 * every plane unit by unit with the units the last search left on the device (svtgpu_lr_search_frame_async: a plane
 * whose frame type came out NONE holds NONE units, which are copied) -- no host round trip between search and apply. */
int  svtgpu_lr_apply_frame(SvtGpuLrState *s, const SvtGpuFrame *deblocked, const SvtGpuFrame *cdef_out,
                           SvtGpuFrame *out, const int32_t frame_type[3], void *stream);


/* Loop-restoration search controls (WnFilterCtrls / SgFilterCtrls, EncModeConfig.c:1329-1445, fixed-range SGR
 * search: step_range 16) and the encoder's rate inputs (Macroblock rdmult / restore costs). */
typedef struct SvtGpuLrSearchControls {
    int32_t wn_enabled, wn_use_chroma, wn_filter_tap_lvl, wn_use_refinement, wn_max_one_refinement_step;
    int32_t sg_enabled, sg_use_chroma;
    int32_t sg_start_ep[2], sg_end_ep[2], sg_ep_inc[2], sg_refine[2]; /* [luma, chroma] */
    int32_t rdmult;
    int32_t switchable_restore_cost[3], wiener_restore_cost[2], sgrproj_restore_cost[2];
} SvtGpuLrSearchControls;
/* Per-unit search record (RestUnitSearchInfo, EbRestoration.h:349-360). */
typedef struct SvtGpuLrUnitSearch {
    int64_t        sse[3];        /* NONE, WIENER (INT64_MAX = no filter), SGRPROJ */
    SvtGpuRestUnit wiener, sgrproj; /* best parameters of each type */
} SvtGpuLrUnitSearch;
/* ≙ restoration_seg_search over every segment + rest_finish_search (EbRestorationPick.c:1471-1634) on the CDEF
 * output `recon` against `source`; sets the units of `s` (frame types in frame_type_out[3]) and, if
 * search_out[plane] is non-NULL, returns the per-unit records.  Synchronous. */
int svtgpu_lr_search_frame(SvtGpuLrState *s, const SvtGpuFrame *recon, const SvtGpuFrame *source,
                           const SvtGpuLrSearchControls *ctrls, int32_t frame_type_out[3],
                           SvtGpuLrUnitSearch *const search_out[3], void *stream);
/* The asynchronous form of svtgpu_lr_search_frame (≙ restoration_seg_search + rest_finish_search with no host wait):
 * the search, the per-unit records and the RD finish (rest_finish_search, EbRestorationPick.c:1555-1634) are enqueued
 * on `stream` and set the state's units in stream order; a picture tiled over GPUs sums the records over its
 * communicator on the device first.  Returns without waiting.  svtgpu_lr_apply_frame(..., frame_type = NULL, ...)
 * applies the result in stream order; svtgpu_lr_read_result waits for it and returns the frame types (and a failure
 * of the device search, e.g. a descent's bound, which this call cannot see).  SVTGPU_LR_FINISH=host: the round-5 form
 * (the records read back, the finish on the host, one wait inside this call). */
int svtgpu_lr_search_frame_async(SvtGpuLrState *s, const SvtGpuFrame *recon, const SvtGpuFrame *source,
                                 const SvtGpuLrSearchControls *ctrls, void *stream);
/* Waits for the last asynchronous search of `s` queued on `stream` and returns its frame types (SVTGPU_RESTORE_*);
 * after a synchronous search, or a second call, the last frame types collected.  SVTGPU_ERR_HIP: the device search
 * failed (svtgpu_error_string names it). */
int svtgpu_lr_read_result(SvtGpuLrState *s, int32_t frame_type_out[3], void *stream);
/* The state's units of one plane (the RestorationUnitInfo the frame header / tile coding writes: the last search's
 * picks, NONE units for a plane whose frame type is NONE); waits for an asynchronous search first. */
int svtgpu_lr_read_units(SvtGpuLrState *s, int32_t plane, SvtGpuRestUnit *units_out, void *stream);
/* Diagnostic read-back of the self-guided filter planes the last search of `s` left on the device (no reference
 * counterpart: the reference keeps them in flt0 / flt1 of search_selfguided_restoration).  `slot` counts the eps the
 * search tried on `plane`, in its order (0 .. their number - 1; with sg_filter_lvl 1 slot == ep); *ep_out receives the
 * ep.  flt0 / flt1 (plane width x plane height int16 each, rows contiguous) receive g = flt - (dgd << 4) of the ep's
 * r = 2 and r = 1 pass, every sample of the plane; a pass the ep does not have (sgr_params r == 0) leaves its array
 * untouched.  Waits for an asynchronous search.  SVTGPU_ERR_INVALID_ARG: no search yet, none on this plane, or no
 * such slot. */
int svtgpu_lr_read_sgr_planes(SvtGpuLrState *s, int32_t plane, int32_t slot, int32_t *ep_out, int16_t *flt0,
                              int16_t *flt1, void *stream);
/* Per-unit part of the search for a band of unit rows: the units of unit rows [row_begin[p], row_end[p]) of each
 * searched plane (restoration_seg_search restricted to those units; every unit's search is independent of the
 * others).  Writes those units' records into search_out[p] (arrays of all units of the plane, row-major; other
 * entries untouched); no RD finish and the state's units are not changed.  The multi-GPU split of the search:
 * every rank searches a band, the records are gathered and svtgpu_lr_finish_plane picks on every rank.
 * Synchronous. */
int svtgpu_lr_search_units(SvtGpuLrState *s, const SvtGpuFrame *recon, const SvtGpuFrame *source,
                           const SvtGpuLrSearchControls *ctrls, const int32_t row_begin[3], const int32_t row_end[3],
                           SvtGpuLrUnitSearch *const search_out[3], void *stream);
/* ≙ rest_finish_search of one plane (EbRestorationPick.c:1555-1634): the frame restoration type and the units'
 * types/parameters (copy_unit_info) from the records of all `nunits` units of the plane.  Host only (no device
 * work, usable without a GPU); returns SVTGPU_OK with *frame_type_out = NONE for a plane that is not searched. */
int svtgpu_lr_finish_plane(const SvtGpuLrSearchControls *ctrls, int32_t plane, int32_t nunits,
                           const SvtGpuLrUnitSearch *records, int32_t *frame_type_out, SvtGpuRestUnit *units_out);
/* ≙ rest_finish_search of the whole frame (EbRestorationPick.c:1555-1634): the planes in order over one
 * RestUnitSearchInfo array shared by the planes, as the reference allocates it -- a chroma plane's switchable pass reads
 * luma's entries for a filter type chroma does not search (Wiener level 5 beside self-guided level 1-3: presets 3-9),
 * which svtgpu_lr_finish_plane on one plane alone cannot.  nunits[p] / records[p] / units_out[p] for the searched
 * planes (units_out of the others zeroed when non-NULL).  Host only. */
int svtgpu_lr_finish_frame(const SvtGpuLrSearchControls *ctrls, const int32_t nunits[3],
                           const SvtGpuLrUnitSearch *const records[3], int32_t frame_type_out[3],
                           SvtGpuRestUnit *const units_out[3]);
/* A picture tiled over GPUs (svtgpu_tile_plan): svtgpu_lr_search_frame searches only the units of units[p] = {col0,
 * row0, col1, row1} of each plane, sums the zero-padded per-unit records over `comm` (the gather), and runs the RD
 * finish of every plane on every rank (the same frame types and units everywhere); svtgpu_lr_apply_frame writes only
 * out[p] = {x0, y0, x1, y1} (plane samples), reading the CDEF output 3 samples and the DLF output 3 rows around it.
 * NULL arrays: the whole frame; NULL comm: no exchange. */
int svtgpu_lr_set_tile(SvtGpuLrState *s, const int32_t units[3][4], const int32_t out[3][4], SvtGpuComm *comm);
/* Device-time profile of the searches timed since the previous read, by kernel class: 0 unit sums + Wiener
 * statistics, 1 self-guided filters (sgr_flt_kernel), 2 Wiener descents (wiener_res_kernel), 3 self-guided searches
 * (sgr_res_kernel: moments, seeds and descents), 4 Wiener decomposition and the chosen ep's SSE, 5 unused.  Each
 * launch is timed from its first workgroup's start to its last workgroup's end on the device's 100 MHz
 * s_memrealtime clock (per-launch HIP event packets would cost more than these launches); bytes = algorithmic
 * HBM bytes of the class (compulsory reads/writes of the samples and filter planes the launches touch). */
typedef struct SvtGpuLrProfile {
    int32_t launches[6]; /* totals over `searches` searches */
    float   ms[6];        /* the device clock: first workgroup start to last workgroup end of each launch */
    double  bytes[6];
    int32_t searches;
    float   ms_events[6]; /* HIP events around each launch on its stream (the span rocprofv3's kernel trace reports) */
} SvtGpuLrProfile;
/* enable != 0 turns timing of the following searches on (0 off): a bit mask of the classes to time (bit c =
 * class c; -1 = all); bit 6 also brackets each timed launch with HIP events (ms_events: the span rocprofv3 reports;
 * events between launches can change how the two LR chains interleave, so they are a separate, opt-in bit); bit 7 runs
 * the Wiener chain on the caller's stream after the self-guided one instead of beside it, so every search kernel has the
 * device to itself and its duration is its own (measurement only: slower searches).  `totals` (nullable) first receives the sums over the searches timed since the previous read
 * (untimed classes read 0), which are then reset; reading synchronizes the device.  The timings accumulate on the
 * device: a timed search adds one small launch and no copies or host synchronization. */
int svtgpu_lr_profile(SvtGpuLrState *s, int32_t enable, SvtGpuLrProfile *totals);
/* Host <-> device bytes moved by the frame-level entry points since the last reset (copies and the results read from
 * mapped memory; per-block shims excluded) -- measurement only, no reference counterpart.  reset != 0 zeroes them. */
int svtgpu_transfer_bytes(uint64_t *h2d, uint64_t *d2h, int32_t reset);
/* controls of wn_filter_lvl / sg_filter_lvl (EncModeConfig.c:1329-1445); rate fields are left zero */
int svtgpu_lr_controls_for_level(int32_t wn_level, int32_t sg_level, SvtGpuLrSearchControls *c);

/* ---------------------------------------------------------------------------------------------
 * CCSO, cross-component sample offset: the fork's AVM experiment, EbCcso.c / EbPickccso.c.
 * The fork's encoder never calls it (EbCdefProcess.c:621-623 comment the search and the apply out); these entry points
 * are what an encoder that re-enables it binds.  Geometry as the reference's: every plane's samples are addressed with
 * the luma width as stride (ccso_stride, EbPickccso.c:800), chroma planes are (width >> 1) x (height >> 1) (the
 * unpadded size >> 1, svt_av1_setup_dst_planes, EbDeblockingFilter.c:114-116), the classifier reads the luma plane
 * padded by SVTGPU_CCSO_PAD samples (ext_rec_y, stride width + 2 * SVTGPU_CCSO_PAD), and the filter blocks are
 * 256 x 256 luma / 128 x 128 chroma samples (CCSO_BLK_SIZE 7, EbDefinitions.h:1409), counted on the 8-aligned mode-info
 * grid: nvfb x nhfb (derive_ccso_filter, EbPickccso.c:473-476).
 * --------------------------------------------------------------------------------------------- */
#define SVTGPU_CCSO_PAD 5     /* CCSO_PADDING_SIZE (EbDefinitions.h:1410) */
#define SVTGPU_CCSO_LUT 2048  /* CCSO_BAND_NUM * 16 (EbDefinitions.h:1411) */
/* one plane of FrameHeader.ccso_info (EbAv1Structs.h:407-427); filter_offset index (band << 4) + (cls0 << 2) + cls1 */
typedef struct SvtGpuCcsoParams {
    uint8_t enable, bo_only, quant_idx, ext_filter_support, max_band_log2, edge_clf, reserved[2];
    int8_t  filter_offset[SVTGPU_CCSO_LUT];
} SvtGpuCcsoParams;
/* the filter-block grid of a plane (nvfb rows x nhfb columns; the block flags arrays are nvfb * nhfb bytes, row-major) */
int svtgpu_ccso_grid(int32_t width, int32_t height, int32_t plane, int32_t *nvfb, int32_t *nhfb);
/* ≙ the ext_rec_y construction (the copy of EbPickccso.c:907-918 + extend_ccso_border, EbCcso.c:185-201): the luma
 * plane (8- or 16-bit samples, device) into `ext` (device, (height + 10) rows of width + 10 uint16), replicated
 * SVTGPU_CCSO_PAD samples on every side. */
int svtgpu_ccso_extend_luma(const void *luma, int32_t bits, int32_t stride, int32_t width, int32_t height,
                            uint16_t *ext, void *stream);
typedef struct SvtGpuCcsoState SvtGpuCcsoState;
int  svtgpu_ccso_state_create(SvtGpuContext *ctx, int32_t width, int32_t height, SvtGpuCcsoState **out);
void svtgpu_ccso_state_destroy(SvtGpuCcsoState *s);
/* ≙ derive_ccso_filter (EbPickccso.c:464-779) of one plane: every (band-offset-only, filter support, quantization step,
 * edge classifier, band count) configuration trained as the reference trains it, the cheapest kept, then weighed
 * against the unfiltered plane.  ext (device, svtgpu_ccso_extend_luma of the pre-filter luma), org / rec (device,
 * uint16, stride = width).  rdmult as derive_ccso_filter receives it (ccso_search's weighting applied).  Results stay
 * in the state for svtgpu_ccso_apply_plane(..., params = NULL); params_out / flags_out (host, nullable) also receive
 * them (one wait).  A disabled plane reads enable = 0 and zero fields / flags. */
int svtgpu_ccso_search_plane(SvtGpuCcsoState *s, const uint16_t *ext, const uint16_t *org, const uint16_t *rec,
                             int32_t plane, int32_t bit_depth, int32_t rdmult, SvtGpuCcsoParams *params_out,
                             uint8_t *flags_out, void *stream);
/* ≙ ccso_search (EbPickccso.c:785-815): rdmult weighted by clamp(base_q_idx, 1, 63), the three planes searched side by
 * side (one launch per pass).  Returns 1 and searches nothing when the weighted rdmult reaches INT_MAX (the reference
 * returns early): the state's device result is then cleared in stream order (every plane enable = 0), so a following
 * svtgpu_ccso_apply_plane(..., NULL, ...) filters nothing instead of applying an earlier frame's search; the host
 * outputs are left as they were.  *frame_flag = ccso_frame_flag (any plane enabled).  params_out = NULL: nothing is read back and
 * nothing waited for (*frame_flag = 0); the results stay in the state for svtgpu_ccso_apply_plane(..., NULL, ...). */
int svtgpu_ccso_search_frame(SvtGpuCcsoState *s, const uint16_t *ext, const uint16_t *const org[3],
                             const uint16_t *const rec[3], int32_t bit_depth, int32_t rdmult, int32_t base_q_idx,
                             SvtGpuCcsoParams params_out[3], uint8_t *const flags_out[3], int32_t *frame_flag,
                             void *stream);
/* ≙ ccso_frame's body for one plane (EbCcso.c:637-677 with ccso_apply_{luma,chroma}_{mb,sb}_filter, :297-622): the
 * plane at `dst` (device, 8- or 16-bit samples, dst_stride samples) offset in place where the block flag is set,
 * classified on `ext`.  params (host) + flags (host, nvfb * nhfb): those; params = NULL: the state's last search of
 * this plane (stream order, no host wait).  A plane with enable = 0 is left as it is. */
int svtgpu_ccso_apply_plane(SvtGpuCcsoState *s, const uint16_t *ext, int32_t plane, int32_t bit_depth, void *dst,
                            int32_t dst_bits, int32_t dst_stride, const SvtGpuCcsoParams *params,
                            const uint8_t *flags, void *stream);
/* per-block RTCD shims (common_dsp_rtcd.h:1025-1090; host pointers, synchronous) */
uint64_t svtgpu_compute_distortion_block(const uint16_t *org, const int org_stride, const uint16_t *rec16,
                                         const int rec_stride, const int x, const int y,
                                         const int log2_filter_unit_size, const int height, const int width);
void svtgpu_ccso_derive_src_block(const uint16_t *src_y, uint8_t *const src_cls0, uint8_t *const src_cls1,
                                  const int src_y_stride, const int ccso_stride, const int x, const int y,
                                  const int pic_width, const int pic_height, const int y_uv_hscale,
                                  const int y_uv_vscale, const int qstep, const int neg_qstep, const int *src_loc,
                                  const int blk_size, const int edge_clf);
void svtgpu_ccso_filter_block_hbd_with_buf(const uint16_t *src_y, uint16_t *dst_yuv, const uint8_t *src_cls0,
                                           const uint8_t *src_cls1, const int src_y_stride, const int dst_stride,
                                           const int ccso_stride, const int x, const int y, const int pic_width,
                                           const int pic_height, const int8_t *filter_offset, const int blk_size,
                                           const int y_uv_hscale, const int y_uv_vscale, const int max_val,
                                           const uint8_t shift_bits, const uint8_t ccso_bo_only);
void svtgpu_ccso_filter_block_hbd_wo_buf(const uint16_t *src_y, uint16_t *dst_yuv, const int x, const int y,
                                         const int pic_width, const int pic_height, int *src_cls,
                                         const int8_t *offset_buf, const int src_y_stride, const int dst_stride,
                                         const int y_uv_hscale, const int y_uv_vscale, const int thr,
                                         const int neg_thr, const int *src_loc, const int max_val, const int blk_size,
                                         const bool isSingleBand, const uint8_t shift_bits, const int edge_clf,
                                         const uint8_t ccso_bo_only);

#ifdef __cplusplus
}
#endif
#endif /* SVTGPU_H */
