"""ctypes binding of libsvtgpu (the MI355X C ABI declared in include/svtgpu.h).

Host-side mirror of the reference's CDEF frame pipeline surface (EbCdefProcess.c /
EbEncCdef.c): search -> pick -> apply on device-resident 4:2:0 frames.  This module is what
tests/ and bench.py call; it never falls back to a CPU path — if the HIP library is missing or no
gfx950 device is visible, it raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVTGPU_LIB") or os.path.join(_HERE, "lib", "libsvtgpu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "svtgpu.h")

SVTGPU_OK = 0
TOTAL_STRENGTHS = 64
MAX_STRENGTHS = 16


class CdefList(ctypes.Structure):
    _fields_ = [("by", ctypes.c_uint8), ("bx", ctypes.c_uint8)]


class CdefControls(ctypes.Structure):
    """SvtGpuCdefControls (mirror of CdefControls, EbPictureControlSet.h:592-628)."""
    _fields_ = [
        ("first_pass_fs_num", ctypes.c_uint8),
        ("default_second_pass_fs_num", ctypes.c_uint8),
        ("default_first_pass_fs", ctypes.c_uint8 * TOTAL_STRENGTHS),
        ("default_second_pass_fs", ctypes.c_uint8 * TOTAL_STRENGTHS),
        ("default_first_pass_fs_uv", ctypes.c_int8 * TOTAL_STRENGTHS),
        ("default_second_pass_fs_uv", ctypes.c_int8 * TOTAL_STRENGTHS),
        ("subsampling_factor", ctypes.c_uint8),
        ("zero_fs_cost_bias", ctypes.c_uint16),
        ("use_reference_cdef_fs", ctypes.c_int8),
        ("pred_y_f", ctypes.c_int8),
        ("pred_uv_f", ctypes.c_int8),
    ]

    def strengths(self):
        n1, n2 = self.first_pass_fs_num, self.default_second_pass_fs_num
        return list(self.default_first_pass_fs[:n1]) + list(self.default_second_pass_fs[:n2])


class CdefParams(ctypes.Structure):
    """SvtGpuCdefParams (mirror of CdefParams, EbAv1Structs.h:359-369)."""
    _fields_ = [
        ("cdef_damping", ctypes.c_uint8),
        ("cdef_bits", ctypes.c_uint8),
        ("cdef_y_strength", ctypes.c_uint8 * MAX_STRENGTHS),
        ("cdef_uv_strength", ctypes.c_uint8 * MAX_STRENGTHS),
    ]

    def as_tuple(self):
        nb = 1 << self.cdef_bits
        return (self.cdef_damping, self.cdef_bits, tuple(self.cdef_y_strength[:nb]),
                tuple(self.cdef_uv_strength[:nb]))


class LfMi(ctypes.Structure):
    """SvtGpuLfMi: the MbModeInfo.block_mi fields the deblocking filter reads (one per 4x4 mi)."""
    _fields_ = [("bsize", ctypes.c_uint8), ("tx_depth", ctypes.c_uint8), ("skip", ctypes.c_uint8),
                ("ref_frame0", ctypes.c_int8), ("mode", ctypes.c_uint8), ("segment_id", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 2)]


LF_MI_DTYPE = np.dtype([("bsize", np.uint8), ("tx_depth", np.uint8), ("skip", np.uint8), ("ref_frame0", np.int8),
                        ("mode", np.uint8), ("segment_id", np.uint8), ("pad", np.uint8, 2)])


class LfParams(ctypes.Structure):
    """SvtGpuLfParams (struct LoopFilter, EbDefinitions.h:1903-1920, + segmentation features)."""
    _fields_ = [
        ("filter_level", ctypes.c_int32 * 2),
        ("filter_level_u", ctypes.c_int32),
        ("filter_level_v", ctypes.c_int32),
        ("sharpness_level", ctypes.c_int32),
        ("mode_ref_delta_enabled", ctypes.c_uint8),
        ("ref_deltas", ctypes.c_int8 * 8),
        ("mode_deltas", ctypes.c_int8 * 2),
        ("segmentation_enabled", ctypes.c_uint8),
        ("seg_feature_data", (ctypes.c_int16 * 8) * 8),
        ("seg_feature_enabled", (ctypes.c_int16 * 8) * 8),
    ]

    def levels(self):
        return (self.filter_level[0], self.filter_level[1], self.filter_level_u, self.filter_level_v)

    @classmethod
    def make(cls, fl0, fl1, flu, flv, sharpness=0, ref_deltas=None, mode_deltas=None, seg_enabled=None,
             seg_data=None):
        """Build from plain values; ref_deltas/mode_deltas given => mode_ref_delta_enabled."""
        p = cls()
        p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v = fl0, fl1, flu, flv
        p.sharpness_level = sharpness
        if ref_deltas is not None:
            p.mode_ref_delta_enabled = 1
            for i, v in enumerate(ref_deltas):
                p.ref_deltas[i] = int(v)
            for i, v in enumerate(mode_deltas if mode_deltas is not None else (0, 0)):
                p.mode_deltas[i] = int(v)
        if seg_enabled is not None:
            p.segmentation_enabled = 1
            for s in range(8):
                for f in range(8):
                    p.seg_feature_enabled[s][f] = int(seg_enabled[s][f])
                    p.seg_feature_data[s][f] = int(seg_data[s][f])
        return p


class DlfByQ(ctypes.Structure):
    """SvtGpuDlfByQ: what svt_av1_pick_filter_level_by_q reads (EbDeblockingFilter.c:1036-1125)."""
    _fields_ = [("bit_depth", ctypes.c_int32), ("base_q_idx", ctypes.c_int32), ("frame_type", ctypes.c_int32),
                ("slice_type", ctypes.c_int32), ("temporal_layer_index", ctypes.c_int32),
                ("ppcs_temporal_layer_index", ctypes.c_int32), ("input_resolution", ctypes.c_int32),
                ("zero_filter_strength_lvl", ctypes.c_int32), ("b64_count", ctypes.c_int32),
                ("me_sad", ctypes.POINTER(ctypes.c_uint32)), ("nref", ctypes.c_int32),
                ("ref_levels", (ctypes.c_int32 * 4) * 7)]


def dlf_pick_by_q(bit_depth, base_q_idx, frame_type, slice_type, temporal_layer_index, ppcs_temporal_layer_index,
                  input_resolution, zero_filter_strength_lvl, me_sad, ref_levels):
    """svtgpu_dlf_pick_by_q (host): LfParams levels (y0, y1, u, v) from the quantizer, no search."""
    me = np.ascontiguousarray(me_sad, np.uint32)
    a = DlfByQ(bit_depth, base_q_idx, frame_type, slice_type, temporal_layer_index, ppcs_temporal_layer_index,
               input_resolution, zero_filter_strength_lvl, len(me), me.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
               len(ref_levels))
    for i, lv in enumerate(ref_levels):
        for k in range(4):
            a.ref_levels[i][k] = int(lv[k])
    out = (ctypes.c_int32 * 4)()
    check(lib().svtgpu_dlf_pick_by_q(ctypes.byref(a), out))
    return tuple(out)


def dlf_qp_based_param(bit_depth, base_q_idx, frame_type):
    y, uv = ctypes.c_int32(), ctypes.c_int32()
    check(lib().svtgpu_dlf_qp_based_param(bit_depth, base_q_idx, frame_type, ctypes.byref(y), ctypes.byref(uv)))
    return y.value, uv.value


class RestUnit(ctypes.Structure):
    """SvtGpuRestUnit (RestorationUnitInfo, EbRestoration.h:169-188)."""
    _fields_ = [("type", ctypes.c_int32), ("vfilter", ctypes.c_int16 * 8), ("hfilter", ctypes.c_int16 * 8),
                ("ep", ctypes.c_int32), ("xqd", ctypes.c_int32 * 2)]


REST_UNIT_DTYPE = np.dtype([("type", np.int32), ("vfilter", np.int16, 8), ("hfilter", np.int16, 8), ("ep", np.int32),
                            ("xqd", np.int32, 2)])


def rest_units_from_rows(rows):
    """[n][20] int32 rows {type, vfilter[8], hfilter[8], ep, xqd0, xqd1} -> REST_UNIT_DTYPE array."""
    rows = np.asarray(rows)
    u = np.zeros(len(rows), REST_UNIT_DTYPE)
    u["type"] = rows[:, 0]
    u["vfilter"] = rows[:, 1:9]
    u["hfilter"] = rows[:, 9:17]
    u["ep"] = rows[:, 17]
    u["xqd"] = rows[:, 18:20]
    return u


class LrSearchControls(ctypes.Structure):
    """SvtGpuLrSearchControls (WnFilterCtrls / SgFilterCtrls + Macroblock rate fields)."""
    _fields_ = [("wn_enabled", ctypes.c_int32), ("wn_use_chroma", ctypes.c_int32), ("wn_filter_tap_lvl", ctypes.c_int32),
                ("wn_use_refinement", ctypes.c_int32), ("wn_max_one_refinement_step", ctypes.c_int32),
                ("sg_enabled", ctypes.c_int32), ("sg_use_chroma", ctypes.c_int32),
                ("sg_start_ep", ctypes.c_int32 * 2), ("sg_end_ep", ctypes.c_int32 * 2),
                ("sg_ep_inc", ctypes.c_int32 * 2), ("sg_refine", ctypes.c_int32 * 2), ("rdmult", ctypes.c_int32),
                ("switchable_restore_cost", ctypes.c_int32 * 3), ("wiener_restore_cost", ctypes.c_int32 * 2),
                ("sgrproj_restore_cost", ctypes.c_int32 * 2)]


LR_PROFILE_DTYPE = np.dtype([("launches", np.int32, 6), ("ms", np.float32, 6), ("bytes", np.float64, 6),
                             ("searches", np.int32), ("ms_events", np.float32, 6)], align=True)
LR_UNIT_SEARCH_DTYPE = np.dtype([("sse", np.int64, 3), ("wiener", REST_UNIT_DTYPE), ("sgrproj", REST_UNIT_DTYPE)],
                                align=True)


class CcsoParams(ctypes.Structure):
    """SvtGpuCcsoParams: one plane of FrameHeader.ccso_info (EbAv1Structs.h:407-427)."""
    _fields_ = [("enable", ctypes.c_uint8), ("bo_only", ctypes.c_uint8), ("quant_idx", ctypes.c_uint8),
                ("ext_filter_support", ctypes.c_uint8), ("max_band_log2", ctypes.c_uint8), ("edge_clf", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 2), ("filter_offset", ctypes.c_int8 * 2048)]

    FIELDS = ("enable", "bo_only", "quant_idx", "ext_filter_support", "max_band_log2", "edge_clf")

    @classmethod
    def make(cls, fields, lut):
        p = cls()
        for n, v in zip(cls.FIELDS, fields):
            setattr(p, n, int(v))
        ctypes.memmove(p.filter_offset, np.ascontiguousarray(lut, dtype=np.int8).ctypes.data, 2048)
        return p

    def fields(self):
        return tuple(int(getattr(self, n)) for n in self.FIELDS)

    def lut(self):
        return np.frombuffer(bytes(self.filter_offset), dtype=np.int8).copy()


class ConvolveParams(ctypes.Structure):
    """SvtGpuConvolveParams: the reference's ConvolveParams layout (EbDefinitions.h:577-590)."""
    _fields_ = [("ref", ctypes.c_int32), ("do_average", ctypes.c_int32), ("dst", ctypes.c_void_p),
                ("dst_stride", ctypes.c_int32), ("round_0", ctypes.c_int32), ("round_1", ctypes.c_int32),
                ("plane", ctypes.c_int32), ("is_compound", ctypes.c_int32), ("use_jnt_comp_avg", ctypes.c_int32),
                ("fwd_offset", ctypes.c_int32), ("bck_offset", ctypes.c_int32),
                ("use_dist_wtd_comp_avg", ctypes.c_int32)]


class SgrParams(ctypes.Structure):
    """SvtGpuSgrParams: the reference's SgrParamsType (EbDefinitions.h:1768-1771)."""
    _fields_ = [("r", ctypes.c_int32 * 2), ("s", ctypes.c_int32 * 2)]


MD_SIZES = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64),
            (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64),
            (64, 16)]
MD_BLOCKS = 849

_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_U64 = ctypes.c_uint64
_U8P = ctypes.POINTER(ctypes.c_uint8)
_LPF8 = (None, [_P, _I32, _P, _P, _P])
_LPF16 = (None, [_P, _I32, _P, _P, _P, _I32])
class TfBlock(ctypes.Structure):
    """Mirror of SvtGpuTfBlock: what the temporal filter's search left for one (reference, 64x64 block)."""
    _fields_ = [("split32", _I32 * 4), ("mv32_x", ctypes.c_int16 * 4), ("mv32_y", ctypes.c_int16 * 4),
                ("mv16_x", ctypes.c_int16 * 16), ("mv16_y", ctypes.c_int16 * 16), ("err32", ctypes.c_uint64 * 4),
                ("err16", ctypes.c_uint64 * 16)]

    @classmethod
    def make(cls, split32, mv32, mv16, err32, err16):
        """mv32 [4][2], mv16 [16][2] as (x, y)."""
        b = cls()
        for i in range(4):
            b.split32[i], b.mv32_x[i], b.mv32_y[i], b.err32[i] = int(split32[i]), int(mv32[i][0]), int(mv32[i][1]), int(err32[i])
        for i in range(16):
            b.mv16_x[i], b.mv16_y[i], b.err16[i] = int(mv16[i][0]), int(mv16[i][1]), int(err16[i])
        return b


class TfParams(ctypes.Structure):
    """Mirror of SvtGpuTfParams."""
    _fields_ = [("decay_factor_fp16", ctypes.c_uint32 * 3), ("mv_dist_th", _I32), ("tf_chroma", _I32), ("bit_depth", _I32),
                ("use_zz_based_filter", _I32)]

    @classmethod
    def make(cls, decay, mv_dist_th, tf_chroma, bit_depth, zz=0):
        p = cls()
        for i in range(3):
            p.decay_factor_fp16[i] = int(decay[i])
        p.mv_dist_th, p.tf_chroma, p.bit_depth, p.use_zz_based_filter = int(mv_dist_th), int(tf_chroma), int(bit_depth), int(zz)
        return p


class TfPlanes(ctypes.Structure):
    """Mirror of SvtGpuTfPlanes: three device pointers and their strides in samples."""
    _fields_ = [("plane", _P * 3), ("stride", _I32 * 3)]

    @classmethod
    def make(cls, ptrs, strides):
        p = cls()
        for i in range(3):
            p.plane[i], p.stride[i] = ptrs[i], int(strides[i])
        return p


class TfMotion(ctypes.Structure):
    """Mirror of SvtGpuTfMotion: the partition and MVs of one (reference, 64x64 block), 368 bytes."""
    _fields_ = [("mv64_x", ctypes.c_int16), ("mv64_y", ctypes.c_int16), ("use64", ctypes.c_uint8),
                ("reserved0", ctypes.c_uint8 * 3), ("split32", ctypes.c_uint8 * 4), ("split16", ctypes.c_uint8 * 16),
                ("reserved1", ctypes.c_uint8 * 4), ("mv32_x", ctypes.c_int16 * 4), ("mv32_y", ctypes.c_int16 * 4),
                ("mv16_x", ctypes.c_int16 * 16), ("mv16_y", ctypes.c_int16 * 16), ("mv8_x", ctypes.c_int16 * 64),
                ("mv8_y", ctypes.c_int16 * 64)]

    @classmethod
    def make(cls, use64, mv64, split32, split16, mv32, mv16, mv8):
        """mv64 (x, y); mv32 [4][2], mv16 [16][2], mv8 [64][2] as (x, y)."""
        m = cls()
        m.use64, m.mv64_x, m.mv64_y = int(use64), int(mv64[0]), int(mv64[1])
        for i in range(4):
            m.split32[i], m.mv32_x[i], m.mv32_y[i] = int(split32[i]), int(mv32[i][0]), int(mv32[i][1])
        for i in range(16):
            m.split16[i], m.mv16_x[i], m.mv16_y[i] = int(split16[i]), int(mv16[i][0]), int(mv16[i][1])
        for i in range(64):
            m.mv8_x[i], m.mv8_y[i] = int(mv8[i][0]), int(mv8[i][1])
        return m


assert ctypes.sizeof(TfMotion) == 368


class TfFullpel(ctypes.Structure):
    """Mirror of SvtGpuTfFullpel: the full-pel MVs ME left for one (reference, 64x64 block) and force64, 352 bytes."""
    _fields_ = [("mv64_x", ctypes.c_int16), ("mv64_y", ctypes.c_int16), ("mv32_x", ctypes.c_int16 * 4),
                ("mv32_y", ctypes.c_int16 * 4), ("mv16_x", ctypes.c_int16 * 16), ("mv16_y", ctypes.c_int16 * 16),
                ("mv8_x", ctypes.c_int16 * 64), ("mv8_y", ctypes.c_int16 * 64), ("force64", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 11)]

    @classmethod
    def make(cls, mv64, mv32, mv16, mv8, force64=0):
        """mv64 (x, y); mv32 [4][2], mv16 [16][2], mv8 [64][2] as (x, y), whole samples."""
        f = cls()
        f.mv64_x, f.mv64_y, f.force64 = int(mv64[0]), int(mv64[1]), int(force64)
        for i in range(4):
            f.mv32_x[i], f.mv32_y[i] = int(mv32[i][0]), int(mv32[i][1])
        for i in range(16):
            f.mv16_x[i], f.mv16_y[i] = int(mv16[i][0]), int(mv16[i][1])
        for i in range(64):
            f.mv8_x[i], f.mv8_y[i] = int(mv8[i][0]), int(mv8[i][1])
        return f


class TfSearchParams(ctypes.Structure):
    """Mirror of SvtGpuTfSearchParams, 40 bytes."""
    _fields_ = [("half_pel_mode", _I32), ("quarter_pel_mode", _I32), ("eight_pel_mode", _I32), ("use_2tap", _I32),
                ("sub_sampling_shift", _I32), ("enable_8x8_pred", _I32), ("subpel_early_exit_th", _I32), ("bit_depth", _I32),
                ("pred_error_32x32_th", ctypes.c_uint64)]

    @classmethod
    def make(cls, modes, use_2tap, sub_sampling_shift, enable_8x8_pred, subpel_early_exit_th, pred_error_32x32_th, bit_depth):
        p = cls()
        p.half_pel_mode, p.quarter_pel_mode, p.eight_pel_mode = (int(v) for v in modes)
        p.use_2tap, p.sub_sampling_shift, p.enable_8x8_pred = int(use_2tap), int(sub_sampling_shift), int(enable_8x8_pred)
        p.subpel_early_exit_th, p.pred_error_32x32_th, p.bit_depth = int(subpel_early_exit_th), int(pred_error_32x32_th), int(bit_depth)
        return p


assert ctypes.sizeof(TfFullpel) == 352 and ctypes.sizeof(TfSearchParams) == 40 and ctypes.sizeof(TfBlock) == 256
_I16P = ctypes.POINTER(ctypes.c_int16)
_CONVOLVE_SR = [_P, _I32, _P, _I32, _I32, _I32, _I16P, _I16P, _I32, _I32]
INTERP_FORMS = ("2d_sr", "x_sr", "y_sr", "2d_copy_sr")
_U16P = ctypes.POINTER(ctypes.c_uint16)
# ... conv_dst, conv_dst_stride, do_average, use_jnt_comp_avg, fwd_offset, bck_offset
_CONVOLVE_JNT = _CONVOLVE_SR + [_P, _I32, _I32, _I32, _I32, _I32]
COMPOUND_FORMS = ("2d_copy", "x", "y", "2d")  # by (phase_x != 0) | (phase_y != 0) << 1


class CompoundBlock(ctypes.Structure):
    """Mirror of SvtGpuCompoundBlock: one bi-predicted block, 32 bytes."""
    _fields_ = [("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w_log2", ctypes.c_uint8), ("h_log2", ctypes.c_uint8),
                ("ref0", ctypes.c_uint8), ("ref1", ctypes.c_uint8), ("mv0_x", ctypes.c_int16), ("mv0_y", ctypes.c_int16),
                ("mv1_x", ctypes.c_int16), ("mv1_y", ctypes.c_int16), ("filter_x", ctypes.c_uint8),
                ("filter_y", ctypes.c_uint8), ("dist_wtd", ctypes.c_uint8), ("fwd_offset", ctypes.c_uint8),
                ("bck_offset", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 11)]

    @classmethod
    def make(cls, x, y, w, h, ref0, ref1, mv0, mv1, filter_x, filter_y, dist_wtd=0, fwd_offset=0, bck_offset=0):
        """w, h: luma size in samples (powers of two); mv0 / mv1 (x, y) in 1/8 luma sample."""
        b = cls()
        b.x, b.y, b.w_log2, b.h_log2 = int(x), int(y), int(w).bit_length() - 1, int(h).bit_length() - 1
        b.ref0, b.ref1, b.mv0_x, b.mv0_y, b.mv1_x, b.mv1_y = int(ref0), int(ref1), int(mv0[0]), int(mv0[1]), int(mv1[0]), int(mv1[1])
        b.filter_x, b.filter_y, b.dist_wtd = int(filter_x), int(filter_y), int(dist_wtd)
        b.fwd_offset, b.bck_offset = int(fwd_offset), int(bck_offset)
        return b


assert ctypes.sizeof(CompoundBlock) == 32


class MaskedCompoundBlock(ctypes.Structure):
    """Mirror of SvtGpuMaskedCompoundBlock: one masked bi-predicted block, 32 bytes; the first 18 as CompoundBlock."""
    _fields_ = [("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w_log2", ctypes.c_uint8), ("h_log2", ctypes.c_uint8),
                ("ref0", ctypes.c_uint8), ("ref1", ctypes.c_uint8), ("mv0_x", ctypes.c_int16), ("mv0_y", ctypes.c_int16),
                ("mv1_x", ctypes.c_int16), ("mv1_y", ctypes.c_int16), ("filter_x", ctypes.c_uint8),
                ("filter_y", ctypes.c_uint8), ("comp_type", ctypes.c_uint8), ("wedge_index", ctypes.c_uint8),
                ("wedge_sign", ctypes.c_uint8), ("mask_type", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 10)]

    @classmethod
    def make(cls, x, y, w, h, ref0, ref1, mv0, mv1, filter_x, filter_y, comp_type, wedge_index=0, wedge_sign=0, mask_type=0):
        """w, h: luma size in samples (powers of two); mv0 / mv1 (x, y) in 1/8 luma sample; comp_type 0 COMPOUND_WEDGE,
        1 COMPOUND_DIFFWTD."""
        b = cls()
        b.x, b.y, b.w_log2, b.h_log2 = int(x), int(y), int(w).bit_length() - 1, int(h).bit_length() - 1
        b.ref0, b.ref1, b.mv0_x, b.mv0_y, b.mv1_x, b.mv1_y = int(ref0), int(ref1), int(mv0[0]), int(mv0[1]), int(mv1[0]), int(mv1[1])
        b.filter_x, b.filter_y, b.comp_type = int(filter_x), int(filter_y), int(comp_type)
        b.wedge_index, b.wedge_sign, b.mask_type = int(wedge_index), int(wedge_sign), int(mask_type)
        return b


assert ctypes.sizeof(MaskedCompoundBlock) == 32 and MaskedCompoundBlock.filter_y.offset == CompoundBlock.filter_y.offset

class WarpBlock(ctypes.Structure):
    """Mirror of SvtGpuWarpBlock: one warped block, 64 bytes."""
    _fields_ = [("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w_log2", ctypes.c_uint8), ("h_log2", ctypes.c_uint8),
                ("ref0", ctypes.c_uint8), ("ref1", ctypes.c_uint8), ("dist_wtd", ctypes.c_uint8),
                ("fwd_offset", ctypes.c_uint8), ("bck_offset", ctypes.c_uint8), ("reserved0", ctypes.c_uint8),
                ("wmmat0", ctypes.c_int32 * 6), ("wmmat1", ctypes.c_int32 * 6), ("reserved", ctypes.c_uint8 * 4)]

    @classmethod
    def make(cls, x, y, w, h, ref0, wmmat0, ref1=0xFF, wmmat1=None, dist_wtd=0, fwd_offset=0, bck_offset=0):
        """w, h: luma size in samples (powers of two); wmmat0 / wmmat1: six model values each; ref1 0xFF: one reference."""
        b = cls()
        b.x, b.y, b.w_log2, b.h_log2 = int(x), int(y), int(w).bit_length() - 1, int(h).bit_length() - 1
        b.ref0, b.ref1, b.dist_wtd, b.fwd_offset, b.bck_offset = int(ref0), int(ref1), int(dist_wtd), int(fwd_offset), int(bck_offset)
        for k in range(6):
            b.wmmat0[k] = int(wmmat0[k])
            b.wmmat1[k] = int(wmmat1[k]) if wmmat1 is not None else 0
        return b


assert ctypes.sizeof(WarpBlock) == 64 and WarpBlock.wmmat0.offset == 12 and WarpBlock.wmmat1.offset == 36


class ObmcNeighbour(ctypes.Structure):
    """Mirror of SvtGpuObmcNeighbour: one overlappable neighbour span, 8 bytes."""
    _fields_ = [("rel", ctypes.c_uint8), ("size", ctypes.c_uint8), ("ref", ctypes.c_uint8), ("filters", ctypes.c_uint8),
                ("mv_x", ctypes.c_int16), ("mv_y", ctypes.c_int16)]


class ObmcBlock(ctypes.Structure):
    """Mirror of SvtGpuObmcBlock: one single-reference block with its above and left neighbour lists, 96 bytes."""
    _fields_ = [("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w_log2", ctypes.c_uint8), ("h_log2", ctypes.c_uint8),
                ("ref", ctypes.c_uint8), ("filter_x", ctypes.c_uint8), ("filter_y", ctypes.c_uint8), ("n_above", ctypes.c_uint8),
                ("n_left", ctypes.c_uint8), ("reserved0", ctypes.c_uint8), ("mv_x", ctypes.c_int16), ("mv_y", ctypes.c_int16),
                ("wm_offset", ctypes.c_int32), ("reserved", ctypes.c_uint8 * 12), ("nb", ObmcNeighbour * 8)]

    @classmethod
    def make(cls, x, y, w, h, ref, mv, filter_x, filter_y, above=(), left=()):
        """w, h: luma size in samples; mv (x, y) in 1/8 luma sample; above / left: up to four spans each, dicts with rel,
        size (units of 4 luma samples), ref, fx, fy, mv."""
        b = cls()
        b.x, b.y, b.w_log2, b.h_log2 = int(x), int(y), int(w).bit_length() - 1, int(h).bit_length() - 1
        b.ref, b.filter_x, b.filter_y, b.mv_x, b.mv_y = int(ref), int(filter_x), int(filter_y), int(mv[0]), int(mv[1])
        b.n_above, b.n_left = len(above), len(left)
        for base, spans in ((0, above), (4, left)):
            for k, n in enumerate(spans[:4]):
                q = b.nb[base + k]
                q.rel, q.size, q.ref, q.filters = int(n["rel"]), int(n["size"]), int(n["ref"]), int(n["fx"]) | int(n["fy"]) << 4
                q.mv_x, q.mv_y = int(n["mv"][0]), int(n["mv"][1])
        return b


assert ctypes.sizeof(ObmcNeighbour) == 8 and ctypes.sizeof(ObmcBlock) == 96 and ObmcBlock.nb.offset == 32


class InterIntraBlock(ctypes.Structure):
    """Mirror of SvtGpuInterIntraBlock: one single-reference inter-intra block, 32 bytes."""
    _fields_ = [("x", ctypes.c_int16), ("y", ctypes.c_int16), ("w_log2", ctypes.c_uint8), ("h_log2", ctypes.c_uint8),
                ("ref", ctypes.c_uint8), ("filter_x", ctypes.c_uint8), ("filter_y", ctypes.c_uint8), ("mode", ctypes.c_uint8),
                ("use_wedge", ctypes.c_uint8), ("wedge_index", ctypes.c_uint8), ("mv_x", ctypes.c_int16), ("mv_y", ctypes.c_int16),
                ("n_top", ctypes.c_uint8 * 2), ("n_left", ctypes.c_uint8 * 2), ("edge_offset", ctypes.c_int32),
                ("reserved", ctypes.c_uint8 * 8)]

    @classmethod
    def make(cls, x, y, w, h, ref, mv, filter_x, filter_y, mode, use_wedge=0, wedge_index=0, n_top=(0, 0), n_left=(0, 0),
             edge_offset=0):
        """w, h: luma size in samples; mv (x, y) in 1/8 luma sample; mode 0 .. 3 (II_DC / V / H / SMOOTH); n_top / n_left:
        (luma, chroma) counts of neighbour samples; edge_offset: the block's first sample in the edge pool."""
        b = cls()
        b.x, b.y, b.w_log2, b.h_log2 = int(x), int(y), int(w).bit_length() - 1, int(h).bit_length() - 1
        b.ref, b.filter_x, b.filter_y, b.mv_x, b.mv_y = int(ref), int(filter_x), int(filter_y), int(mv[0]), int(mv[1])
        b.mode, b.use_wedge, b.wedge_index, b.edge_offset = int(mode), int(use_wedge), int(wedge_index), int(edge_offset)
        b.n_top[0], b.n_top[1], b.n_left[0], b.n_left[1] = int(n_top[0]), int(n_top[1]), int(n_left[0]), int(n_left[1])
        return b


assert ctypes.sizeof(InterIntraBlock) == 32 and InterIntraBlock.mv_x.offset == 12 and InterIntraBlock.edge_offset.offset == 20
INTRA_KINDS = ("dc", "dc_top", "dc_left", "dc_128", "v", "h", "smooth")

_SIGS = {
    "svtgpu_device_available": (ctypes.c_int, []),
    "svtgpu_version": (ctypes.c_char_p, []),
    "svtgpu_abi_version": (_I32, []),
    "svtgpu_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "svtgpu_context_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    "svtgpu_context_destroy": (None, [_P]),
    "svtgpu_context_stream": (_P, [_P]),
    "svtgpu_synchronize": (ctypes.c_int, [_P, _P]),
    "svtgpu_stream_create": (ctypes.c_int, [_P, _I32, ctypes.POINTER(_P)]),
    "svtgpu_stream_destroy": (None, [_P]),
    "svtgpu_frame_create": (ctypes.c_int, [_P, _I32, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_frame_destroy": (None, [_P]),
    "svtgpu_frame_stride": (_I32, [_P, ctypes.c_int]),
    "svtgpu_frame_plane_ptr": (_P, [_P, ctypes.c_int]),
    "svtgpu_frame_upload": (ctypes.c_int, [_P, ctypes.c_int, _P, _I32, _P]),
    "svtgpu_frame_download": (ctypes.c_int, [_P, ctypes.c_int, _P, _I32, _P]),
    "svtgpu_frame_upload_rect": (ctypes.c_int, [_P, ctypes.c_int, _P, _I32, _P, _P]),
    "svtgpu_frame_copy": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_find_dir": (ctypes.c_uint8, [_P, _I32, ctypes.POINTER(_I32), _I32]),
    "svtgpu_cdef_find_dir_dual": (None, [_P, _P, ctypes.c_int, ctypes.POINTER(_I32), ctypes.POINTER(_I32), _I32,
                                         ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]),
    "svtgpu_cdef_filter_block": (None, [_P, _P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, ctypes.c_uint8]),
    "svtgpu_compute_cdef_dist_16bit": (_U64, [_P, _I32, _P, _P, _I32, _I32, _I32, _I32, ctypes.c_uint8]),
    "svtgpu_compute_cdef_dist_8bit": (_U64, [_P, _I32, _P, _P, _I32, _I32, _I32, _I32, ctypes.c_uint8]),
    "svtgpu_search_one_dual": (_U64, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                      ctypes.POINTER(ctypes.POINTER(ctypes.POINTER(_U64))), ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int]),
    "svtgpu_cdef_controls_for_level": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(CdefControls)]),
    "svtgpu_cdef_state_create": (ctypes.c_int, [_P, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_cdef_state_destroy": (None, [_P]),
    "svtgpu_cdef_state_nfb": (_I32, [_P]),
    "svtgpu_cdef_set_block_mask": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_set_fb_bsize": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_search_frame": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(CdefControls), _I32, _P]),
    "svtgpu_cdef_pick": (ctypes.c_int, [_P, ctypes.POINTER(CdefControls), _I32, _U64, ctypes.POINTER(CdefParams),
                                        _P, _P]),
    "svtgpu_cdef_set_fb_strength": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_apply_frame": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(CdefParams), _P]),
    "svtgpu_cdef_pick_async": (ctypes.c_int, [_P, ctypes.POINTER(CdefControls), _I32, _U64, _P]),
    "svtgpu_cdef_read_params": (ctypes.c_int, [_P, ctypes.POINTER(CdefParams), _P, _P]),
    "svtgpu_cdef_set_fb_rows": (ctypes.c_int, [_P, _I32, _I32]),
    "svtgpu_cdef_bind_tables": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_bind_dir_tables": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_cdef_clear_tables": (ctypes.c_int, [_P, _P]),
    "svtgpu_cdef_read_state": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "svtgpu_cdef_mse_device_ptr": (_P, [_P]),
    **{"svtgpu_lpf_%s_%d" % (d, n): _LPF8 for d in ("horizontal", "vertical") for n in (4, 6, 8, 14)},
    **{"svtgpu_highbd_lpf_%s_%d" % (d, n): _LPF16 for d in ("horizontal", "vertical") for n in (4, 6, 8, 14)},
    "svtgpu_dlf_state_create": (ctypes.c_int, [_P, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_dlf_state_destroy": (None, [_P]),
    "svtgpu_dlf_set_mode_info": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_dlf_set_mode_info_device": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_dlf_frame": (ctypes.c_int, [_P, _P, ctypes.POINTER(LfParams), _I32, _I32, _P]),
    "svtgpu_dlf_frame_to": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LfParams), _I32, _I32, _P]),
    "svtgpu_dlf_pick": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LfParams), _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_dlf_pick_async": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LfParams), _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_dlf_read_levels": (ctypes.c_int, [_P, ctypes.POINTER(LfParams), _P]),
    "svtgpu_dlf_async_rounds": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_dlf_pick_by_q": (ctypes.c_int, [_P, _P]),
    "svtgpu_dlf_qp_based_param": (ctypes.c_int, [_I32, _I32, _I32, _P, _P]),
    "svtgpu_plane_sse": (ctypes.c_int, [_P, _P, _I32, ctypes.POINTER(_U64), _P]),
    **{"svtgpu_aom_sad%dx%d" % s: (ctypes.c_uint32, [_P, ctypes.c_int, _P, ctypes.c_int]) for s in MD_SIZES},
    **{"svtgpu_aom_sad%dx%dx4d" % s: (None, [_P, ctypes.c_int, _P, ctypes.c_int, _P]) for s in MD_SIZES},
    **{"svtgpu_aom_variance%dx%d" % s: (ctypes.c_uint32, [_P, ctypes.c_int, _P, ctypes.c_int,
                                                          ctypes.POINTER(ctypes.c_uint32)]) for s in MD_SIZES},
    **{"svtgpu_aom_highbd_10_variance%dx%d" % s: (ctypes.c_uint32, [_P, ctypes.c_int, _P, ctypes.c_int,
                                                                    ctypes.POINTER(ctypes.c_uint32)])
       for s in MD_SIZES},
    "svtgpu_sad_16b_kernel": (ctypes.c_uint32, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint32]),
    "svtgpu_aom_sse": (ctypes.c_int64, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_aom_highbd_sse": (ctypes.c_int64, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_spatial_full_distortion_kernel": (_U64, [_P, ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_int32,
                                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_full_distortion_kernel16_bits": (_U64, [_P, ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_int32,
                                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_nxm_sad_kernel": (ctypes.c_uint32, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.c_uint32]),
    "svtgpu_nxm_sad_kernel_sub_sampled": (ctypes.c_uint32, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32,
                                                            ctypes.c_uint32]),
    "svtgpu_aom_mse16x16": (ctypes.c_uint32, [_P, _I32, _P, _I32, ctypes.POINTER(ctypes.c_uint32)]),
    "svtgpu_aom_highbd_8_mse16x16": (None, [_P, _I32, _P, _I32, ctypes.POINTER(ctypes.c_uint32)]),
    "svtgpu_aom_variance_highbd": (ctypes.c_uint32, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_uint32)]),
    **{"svtgpu_aom_sub_pixel_variance%dx%d" % s: (ctypes.c_uint32, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P,
                                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)])
       for s in MD_SIZES},
    "svtgpu_cdef_filter_block_8xn_16": (None, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32, ctypes.c_uint8,
                                               ctypes.c_uint8]),
    "svtgpu_aom_copy_rect8_8bit_to_16bit": (None, [_P, _I32, _P, _I32, _I32, _I32]),
    "svtgpu_av1_compute_stats": (None, [_I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "svtgpu_av1_compute_stats_highbd": (None, [_I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32]),
    "svtgpu_av1_lowbd_pixel_proj_error": (ctypes.c_int64, [_P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I32, _P, _P]),
    "svtgpu_av1_highbd_pixel_proj_error": (ctypes.c_int64, [_P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _I32, _P,
                                                            _P]),
    "svtgpu_get_proj_subspace": (None, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int,
                                        _P, ctypes.c_int, _P, ctypes.c_int, _P, _P]),
    "svtgpu_md_batch_create": (ctypes.c_int, [_P, _I32, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_me_batch_create": (ctypes.c_int, [_P, _I32, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_convert_8bit_to_16bit": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_convert_16bit_to_8bit": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_aom_generate_padding": (None, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_uint32]),
    "svtgpu_aom_generate_padding16_bit": (None, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_extend_frame": (None, [_P, _I32, _I32, _I32, _I32, _I32, _I32]),
    "svtgpu_convert_plane": (ctypes.c_int, [_P, _I32, _I32, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_pad_plane": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_extend_plane": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_frame_convert": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_superres_scaled_size": (_I32, [_I32, _I32]),
    "svtgpu_superres_geometry": (ctypes.c_int, [_I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "svtgpu_superres_upscale_plane": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_superres_upscale_frame": (ctypes.c_int, [_P, _P, _I32, _I32, _P]),
    "svtgpu_resize_plan": (ctypes.c_int, [_I32, _I32] + [ctypes.POINTER(_I32)] * 4),
    "svtgpu_resize_filter": (ctypes.c_int, [_I32, _P]),
    "svtgpu_resize_half_filters": (ctypes.c_int, [_P, _P]),
    "svtgpu_resize_plane": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_resize_frame": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_av1_resize_plane": (ctypes.c_uint32, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int]),
    "svtgpu_av1_highbd_resize_plane": (ctypes.c_uint32, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int,
                                                         ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_tf_state_create": (ctypes.c_int, [_P, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_tf_state_destroy": (None, [_P]),
    "svtgpu_tf_estimate_noise": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P, ctypes.POINTER(_I32)]),
    "svtgpu_tf_estimate_noise_async": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_tf_read_noise": (ctypes.c_int, [_P, _P, ctypes.POINTER(_I32)]),
    "svtgpu_tf_filter_frame": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), ctypes.POINTER(TfPlanes), _I32,
                                              ctypes.POINTER(TfBlock), ctypes.POINTER(TfParams), ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_tf_noise_log1p_fp16": (_I32, [_I32]),
    "svtgpu_tf_decay_factor_fp16": (ctypes.c_uint32, [_I32, _I32, _I32]),
    "svtgpu_tf_tables": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(_I32), ctypes.POINTER(_P), ctypes.POINTER(_P),
                                        ctypes.POINTER(_I32)]),
    "svtgpu_estimate_noise_fp16": (_I32, [_P, ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint16]),
    "svtgpu_estimate_noise_highbd_fp16": (_I32, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_tf_apply_planewise_medium": (None, [ctypes.POINTER(TfBlock), _I32, ctypes.POINTER(TfParams)] + [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P,
                                                      ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                      ctypes.c_int] + [_P] * 6),
    "svtgpu_tf_apply_planewise_medium_hbd": (None, [ctypes.POINTER(TfBlock), _I32, ctypes.POINTER(TfParams)] + [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P, ctypes.c_int, _P, _P,
                                                          ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                          ctypes.c_int] + [_P] * 6 + [ctypes.c_uint32]),
    "svtgpu_tf_apply_zz_planewise_medium": (None, [ctypes.POINTER(TfBlock), _I32, ctypes.POINTER(TfParams)] + [_P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_uint,
                                                         ctypes.c_uint, ctypes.c_int, ctypes.c_int] + [_P] * 6),
    "svtgpu_tf_apply_zz_planewise_medium_hbd": (None, [ctypes.POINTER(TfBlock), _I32, ctypes.POINTER(TfParams)] + [_P, ctypes.c_int, _P, _P, ctypes.c_int, ctypes.c_uint,
                                                             ctypes.c_uint, ctypes.c_int, ctypes.c_int] + [_P] * 6 +
                                                [ctypes.c_uint32]),
    "svtgpu_tf_apply_filtering_central": (None, [_I32, _I32, _P, _P, _P, ctypes.c_uint16, ctypes.c_uint16, ctypes.c_uint32,
                                                 ctypes.c_uint32]),
    "svtgpu_tf_apply_filtering_central_highbd": (None, [_I32, _I32, _P, _P, _P, ctypes.c_uint16, ctypes.c_uint16,
                                                        ctypes.c_uint32, ctypes.c_uint32]),
    "svtgpu_tf_get_final_filtered_pixels": (None, [_I32, _P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_uint16,
                                                   ctypes.c_uint16, ctypes.c_int]),
    **{"svtgpu_av1_convolve_" + f: (None, _CONVOLVE_SR) for f in INTERP_FORMS},
    **{"svtgpu_av1_highbd_convolve_" + f: (None, _CONVOLVE_SR + [_I32]) for f in INTERP_FORMS},
    "svtgpu_interp_tables": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(_I32)]),
    "svtgpu_tf_predict_frame": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32, ctypes.POINTER(TfMotion),
                                               _I32, _I32, ctypes.POINTER(TfPlanes), _P]),
    **{"svtgpu_av1_jnt_convolve_" + f: (None, _CONVOLVE_JNT) for f in COMPOUND_FORMS},
    **{"svtgpu_av1_highbd_jnt_convolve_" + f: (None, _CONVOLVE_JNT + [_I32]) for f in COMPOUND_FORMS},
    "svtgpu_dist_wtd_weights": (ctypes.c_int, [_I32, _I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "svtgpu_compound_predict_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32,
                                                     ctypes.POINTER(CompoundBlock), _I32, _I32, _I32,
                                                     ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_av1_build_compound_diffwtd_mask_d16": (None, [_P, _I32, _P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32]),
    "svtgpu_aom_lowbd_blend_a64_d16_mask": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P,
                                                   ctypes.c_uint32, _I32, _I32, _I32, _I32, _I32, _I32]),
    "svtgpu_aom_highbd_blend_a64_d16_mask": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P,
                                                    ctypes.c_uint32, _I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    "svtgpu_wedge_mask": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P]),
    "svtgpu_masked_compound_predict_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32,
                                                            ctypes.POINTER(MaskedCompoundBlock), _I32, _I32, _I32,
                                                            ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_warp_shear_params": (ctypes.c_int, [_P, _P]),
    "svtgpu_warp_filter_table": (ctypes.c_int, [ctypes.POINTER(_P), ctypes.POINTER(_I32)]),
    "svtgpu_av1_warp_affine": (ctypes.c_int, [_P, _P, _I32, _I32, _I32, _P] + [_I32] * 10 + [_P] + [_I32] * 5 + [ctypes.c_int16] * 4),
    "svtgpu_av1_highbd_warp_affine": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P] + [_I32] * 11 + [_P] + [_I32] * 5 +
                                      [ctypes.c_int16] * 4),
    "svtgpu_warp_predict_batch": (ctypes.c_int, [_P, _P, _I32, _P, _I32, _I32, _I32, _P, _P]),
    "svtgpu_obmc_mask": (ctypes.c_int, [_I32, ctypes.POINTER(_P)]),
    **{"svtgpu_aom_blend_a64_%smask" % d: (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, _I32, _I32])
       for d in "vh"},
    **{"svtgpu_aom_highbd_blend_a64_%smask_%s" % (d, f): (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P,
                                                                 _I32, _I32, _I32]) for d in "vh" for f in ("16bit", "8bit")},
    "svtgpu_obmc_weighted_src_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32, _P, _I32,
                                                      ctypes.POINTER(ObmcBlock), _I32, _P, _I32, _P]),
    "svtgpu_obmc_set_items_device_wm": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, ctypes.POINTER(_P), _P]),
    "svtgpu_obmc_predict_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32, ctypes.POINTER(ObmcBlock), _I32,
                                                 _I32, _I32, ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_interintra_smooth_mask": (ctypes.c_int, [_I32, _I32, _I32, _P]),
    "svtgpu_interintra_predict_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32,
                                                       ctypes.POINTER(InterIntraBlock), _I32, _P, _I32, _I32, _I32,
                                                       ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_interintra_mode_sse_batch": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), _I32, _I32, _I32,
                                                        ctypes.POINTER(InterIntraBlock), _I32, _P, _I32, _I32, _P, _I32, _P, _P]),
    "svtgpu_aom_blend_a64_mask": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_aom_highbd_blend_a64_mask": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, ctypes.c_uint32,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_aom_intra_predictor": (None, [_P, ctypes.c_ssize_t, _P, _P, _I32, _I32, _I32]),
    "svtgpu_aom_highbd_intra_predictor": (None, [_P, ctypes.c_ssize_t, _P, _P, _I32, _I32, _I32, _I32]),
    "svtgpu_tf_search_frame": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), ctypes.POINTER(TfPlanes), _I32, _I32, _I32,
                                              ctypes.POINTER(TfFullpel), ctypes.POINTER(TfSearchParams), _P]),
    "svtgpu_tf_search_read": (ctypes.c_int, [_P, _I32, ctypes.POINTER(TfMotion), ctypes.POINTER(TfBlock), _P]),
    "svtgpu_tf_compensate_filter_frame": (ctypes.c_int, [_P, ctypes.POINTER(TfPlanes), ctypes.POINTER(TfPlanes), _I32, _I32,
                                                         _I32, ctypes.POINTER(TfParams), _I32, ctypes.POINTER(TfPlanes),
                                                         ctypes.POINTER(TfPlanes), _P]),
    "svtgpu_me_batch_destroy": (None, [_P]),
    "svtgpu_me_set_origins": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_me_search": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_me_read": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P]),
    **{"svtgpu_aom_obmc_sad%dx%d" % s: (ctypes.c_uint, [_P, ctypes.c_int, _P, _P]) for s in MD_SIZES},
    **{"svtgpu_aom_obmc_variance%dx%d" % s: (ctypes.c_uint, [_P, ctypes.c_int, _P, _P, ctypes.POINTER(ctypes.c_uint)])
       for s in MD_SIZES},
    **{"svtgpu_aom_obmc_sub_pixel_variance%dx%d" % s: (ctypes.c_uint, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P,
                                                                         _P, ctypes.POINTER(ctypes.c_uint)])
       for s in MD_SIZES},
    "svtgpu_obmc_batch_create": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_obmc_batch_destroy": (None, [_P]),
    "svtgpu_obmc_set_items": (ctypes.c_int, [_P, _P, _I32, _P, _I32, _P, _I32, _P]),
    "svtgpu_obmc_search": (ctypes.c_int, [_P, _P, _I32, _I32, _P]),
    "svtgpu_obmc_read": (ctypes.c_int, [_P, _P, _I32, _I32, _P]),
    "svtgpu_ext_all_sad_calculation_8x8_16x16": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32, _P,
                                                        _P, _P, _P, _P, _P, ctypes.c_uint8]),
    "svtgpu_ext_eight_sad_calculation_32x32_64x64": (None, [_P, _P, _P, _P, _P, ctypes.c_uint32, _P]),
    "svtgpu_ext_sad_calculation_8x8_16x16": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P, _P, _P,
                                                    ctypes.c_uint32, _P, _P, ctypes.c_uint8]),
    "svtgpu_ext_sad_calculation_32x32_64x64": (None, [_P, _P, _P, _P, _P, ctypes.c_uint32, _P]),
    "svtgpu_sad_loop_kernel": (None, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P,
                                      _P, _P, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_int16, ctypes.c_int16]),
    "svtgpu_pme_sad_loop_kernel": (None, [_P, _P, ctypes.c_uint32, _P, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, _P, _P, _P, ctypes.c_int16, ctypes.c_int16, ctypes.c_int16,
                                          ctypes.c_int16, ctypes.c_int16, ctypes.c_int16, ctypes.c_int16]),
    "svtgpu_md_batch_destroy": (None, [_P]),
    "svtgpu_md_batch_nsb": (_I32, [_P]),
    "svtgpu_md_set_mvs": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_md_dist_batch": (ctypes.c_int, [_P, _P, _P, _I32, _I32, _P]),
    "svtgpu_md_read": (ctypes.c_int, [_P, _P, _I32, _I32, _P]),
    "svtgpu_md_out_device_ptr": (_P, [_P]),
    "svtgpu_md_moments_device_ptr": (_P, [_P]),
    "svtgpu_md_expand": (ctypes.c_int, [_P, _I32, _I32, _P]),
    "svtgpu_md_layout": (None, [_P, _P, _P]),
    "svtgpu_av1_wiener_convolve_add_src": (None, [_P, ctypes.c_ssize_t, _P, ctypes.c_ssize_t, _P, _P, _I32, _I32,
                                                  ctypes.POINTER(ConvolveParams)]),
    "svtgpu_av1_highbd_wiener_convolve_add_src": (None, [_P, ctypes.c_ssize_t, _P, ctypes.c_ssize_t, _P, _P, _I32,
                                                         _I32, ctypes.POINTER(ConvolveParams), _I32]),
    "svtgpu_av1_selfguided_restoration": (None, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _I32, _I32]),
    "svtgpu_apply_selfguided_restoration": (None, [_P, _I32, _I32, _I32, _I32, _P, _P, _I32, _P, _I32, _I32]),
    "svtgpu_lr_state_create": (ctypes.c_int, [_P, _I32, _I32, _P, ctypes.POINTER(_P)]),
    "svtgpu_lr_state_destroy": (None, [_P]),
    "svtgpu_lr_units": (ctypes.c_int, [_P, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "svtgpu_lr_set_units": (ctypes.c_int, [_P, _I32, _P, _P]),
    "svtgpu_lr_apply_frame": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "svtgpu_lr_search_frame": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LrSearchControls), _P, _P, _P]),
    "svtgpu_lr_controls_for_level": (ctypes.c_int, [_I32, _I32, ctypes.POINTER(LrSearchControls)]),
    "svtgpu_lr_search_units": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LrSearchControls), _P, _P, _P, _P]),
    "svtgpu_lr_finish_plane": (ctypes.c_int, [ctypes.POINTER(LrSearchControls), _I32, _I32, _P, _P, _P]),
    "svtgpu_lr_finish_frame": (ctypes.c_int, [ctypes.POINTER(LrSearchControls), _P, _P, _P, _P]),
    "svtgpu_lr_search_frame_async": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(LrSearchControls), _P]),
    "svtgpu_lr_read_result": (ctypes.c_int, [_P, _P, _P]),
    "svtgpu_lr_read_units": (ctypes.c_int, [_P, _I32, _P, _P]),
    "svtgpu_lr_read_sgr_planes": (ctypes.c_int, [_P, _I32, _I32, ctypes.POINTER(_I32), _P, _P, _P]),
    "svtgpu_lr_profile": (ctypes.c_int, [_P, _I32, _P]),
    "svtgpu_transfer_bytes": (ctypes.c_int, [_P, _P, _I32]),
    "svtgpu_comm_unique_id": (ctypes.c_int, [_P]),
    "svtgpu_comm_create": (ctypes.c_int, [_P, _I32, _I32, _P, ctypes.POINTER(_P)]),
    "svtgpu_comm_create_bounded": (ctypes.c_int, [_P, _I32, _I32, _P, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_comm_create_host": (ctypes.c_int, [_I32, _I32, _P, ctypes.POINTER(_P)]),
    "svtgpu_comm_destroy": (None, [_P]),
    "svtgpu_comm_nranks": (_I32, [_P]),
    "svtgpu_comm_rank": (_I32, [_P]),
    "svtgpu_comm_allreduce_u64": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _I32, _P]),
    "svtgpu_comm_set_timeout": (ctypes.c_int, [_P, _I32]),
    "svtgpu_comm_timeout_ms": (_I32, [_P]),
    "svtgpu_comm_set_slot": (ctypes.c_int, [_P, _I32]),
    "svtgpu_comm_failed": (_I32, [_P]),
    "svtgpu_comm_sync": (ctypes.c_int, [_P, _P]),
    "svtgpu_debug_stall": (ctypes.c_int, [_P, _P, _I32]),
    "svtgpu_shim_calls": (ctypes.c_uint64, []),
    "svtgpu_tile_plan": (ctypes.c_int, [_I32, _I32, _P, _I32, _I32, _I32, _P]),
    "svtgpu_tile_plan_sb": (ctypes.c_int, [_I32, _I32, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_tile_plan_crop": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _I32, _I32, _I32, _I32, _P]),
    "svtgpu_dlf_set_tile": (ctypes.c_int, [_P, _P, _P, _P]),
    "svtgpu_dlf_set_crop": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32]),
    "svtgpu_cdef_set_tile": (ctypes.c_int, [_P, _P, _P, _P]),
    "svtgpu_lr_set_tile": (ctypes.c_int, [_P, _P, _P, _P]),
    "svtgpu_buffer_alloc": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.POINTER(_P)]),
    "svtgpu_buffer_free": (None, [_P]),
    "svtgpu_buffer_upload": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P]),
    "svtgpu_buffer_download": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P]),
    "svtgpu_ccso_grid": (ctypes.c_int, [_I32, _I32, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "svtgpu_ccso_extend_luma": (ctypes.c_int, [_P, _I32, _I32, _I32, _I32, _P, _P]),
    "svtgpu_ccso_state_create": (ctypes.c_int, [_P, _I32, _I32, ctypes.POINTER(_P)]),
    "svtgpu_ccso_state_destroy": (None, [_P]),
    "svtgpu_ccso_search_plane": (ctypes.c_int, [_P, _P, _P, _P, _I32, _I32, _I32, ctypes.POINTER(CcsoParams), _P,
                                                _P]),
    "svtgpu_ccso_search_frame": (ctypes.c_int, [_P, _P, _P * 3, _P * 3, _I32, _I32, _I32, ctypes.POINTER(CcsoParams),
                                                _P, ctypes.POINTER(_I32), _P]),
    "svtgpu_ccso_apply_plane": (ctypes.c_int, [_P, _P, _I32, _I32, _P, _I32, _I32, ctypes.POINTER(CcsoParams), _P,
                                               _P]),
    "svtgpu_compute_distortion_block": (ctypes.c_uint64, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "svtgpu_ccso_derive_src_block": (None, [_P, _P, _P] + [ctypes.c_int] * 10 + [_P, ctypes.c_int, ctypes.c_int]),
    "svtgpu_ccso_filter_block_hbd_with_buf": (None, [_P, _P, _P, _P] + [ctypes.c_int] * 7 + [_P] +
                                              [ctypes.c_int] * 4 + [ctypes.c_uint8, ctypes.c_uint8]),
    "svtgpu_ccso_filter_block_hbd_wo_buf": (None, [_P, _P] + [ctypes.c_int] * 4 + [_P, _P] + [ctypes.c_int] * 6 +
                                            [_P, ctypes.c_int, ctypes.c_int, ctypes.c_bool, ctypes.c_uint8,
                                             ctypes.c_int, ctypes.c_uint8]),
}

_lib = None


def lib():
    """Load libsvtgpu.so (in-tree build).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libsvtgpu.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class SvtGpuError(RuntimeError):
    pass


def check(rc):
    if rc != SVTGPU_OK:
        raise SvtGpuError("svtgpu error %d: %s" % (rc, lib().svtgpu_error_string(rc).decode()))
    return rc


def require_device():
    if not lib().svtgpu_device_available():
        raise SvtGpuError("no gfx950 device visible: the HIP path is required (no CPU fallback)")


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class Context:
    def __init__(self, device=0):
        require_device()
        h = _P()
        check(lib().svtgpu_context_create(device, ctypes.byref(h)))
        self.h = h

    @property
    def stream(self):
        return lib().svtgpu_context_stream(self.h)

    def synchronize(self, stream=None):
        check(lib().svtgpu_synchronize(self.h, stream))

    def stream_create(self, priority=0):
        """A new hipStream_t (as an int) for the frame-level calls: one hardware queue each while the process has no
        more streams than GPU_MAX_HW_QUEUES (svtgpu_stream_create).  Wrap it with torch.cuda.ExternalStream to time
        it with torch events; destroy it with stream_destroy."""
        h = _P()
        check(lib().svtgpu_stream_create(self.h, int(priority), ctypes.byref(h)))
        return h.value

    @staticmethod
    def stream_destroy(stream):
        lib().svtgpu_stream_destroy(stream)

    def debug_stall(self, ms, stream=None):
        """Test support: hold `stream` busy for `ms` milliseconds (one spinning wave)."""
        check(lib().svtgpu_debug_stall(self.h, stream, int(ms)))

    def close(self):
        if self.h:
            lib().svtgpu_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frame:
    """Device-resident 4:2:0 picture (uint8 for 8-bit, uint16 for 10-bit samples)."""

    def __init__(self, ctx, width, height, bit_depth):
        self.ctx, self.width, self.height, self.bit_depth = ctx, width, height, bit_depth
        self.dtype = np.uint16 if bit_depth > 8 else np.uint8
        h = _P()
        check(lib().svtgpu_frame_create(ctx.h, width, height, bit_depth, ctypes.byref(h)))
        self.h = h

    def plane_shape(self, p):
        return (self.height, self.width) if p == 0 else (self.height // 2, self.width // 2)

    def upload(self, planes, stream=None, rect=None):
        """All samples, or (rect = luma {x0, y0, x1, y1}) only those of the rectangle: chroma halved, rounded outward
        (svtgpu_frame_upload_rect; a rank of a tiled picture uploads its plan's in_rect)."""
        keep = []
        for p, a in enumerate(planes):
            a = np.ascontiguousarray(a, dtype=self.dtype)
            assert a.shape == self.plane_shape(p), (a.shape, self.plane_shape(p))
            keep.append(a)
            if rect is None:
                check(lib().svtgpu_frame_upload(self.h, p, ptr(a), a.shape[1], stream))
            else:
                r = chroma_rect(rect, a.shape) if p else [int(v) for v in rect]
                check(lib().svtgpu_frame_upload_rect(self.h, p, ptr(a), a.shape[1], _rect(r), stream))
        self.ctx.synchronize(stream)  # host buffers must outlive the copies

    def download(self, stream=None):
        out = []
        for p in range(3):
            a = np.empty(self.plane_shape(p), dtype=self.dtype)
            check(lib().svtgpu_frame_download(self.h, p, ptr(a), a.shape[1], stream))
            out.append(a)
        return out

    def close(self):
        if self.h:
            lib().svtgpu_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cdef_controls(level):
    c = CdefControls()
    check(lib().svtgpu_cdef_controls_for_level(level, ctypes.byref(c)))
    return c


class TilePlan(ctypes.Structure):
    """SvtGpuTilePlan: what one rank of a picture tiled over GPUs computes (svtgpu_tile_plan)."""
    _fields_ = [("tile", _I32 * 4), ("fb_rect", _I32 * 4), ("lr_units", (_I32 * 4) * 3), ("lr_out", (_I32 * 4) * 3),
                ("cdef_out", _I32 * 4), ("dlf_out", _I32 * 4), ("in_rect", _I32 * 4)]

    def rects(self):
        return {k: (np.array(getattr(self, k)).tolist()) for k, _ in self._fields_}


def chroma_rect(r, shape):
    """A luma rectangle {x0, y0, x1, y1} on a 4:2:0 chroma plane of `shape` (rows, cols): halved, rounded outward."""
    return [int(r[0]) // 2, int(r[1]) // 2, min(shape[1], (int(r[2]) + 1) // 2), min(shape[0], (int(r[3]) + 1) // 2)]


def tile_grid(n):
    """gx x gy of n ranks: the widest split with gx <= gy (1x1, 1x2, 2x2, 2x4 for 1, 2, 4, 8 GPUs)."""
    gx = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return gx, n // gx


def tile_plan(width, height, unit_size, gx, gy, rank, sb=64, crop=None):
    """svtgpu_tile_plan_sb; crop=(w, h): a picture whose crop size is below the 8-aligned coded size width x height
    (svtgpu_tile_plan_crop)."""
    us = np.ascontiguousarray(unit_size, np.int32)
    t = TilePlan()
    if crop is None:
        check(lib().svtgpu_tile_plan_sb(width, height, ptr(us), sb, gx, gy, rank, ctypes.byref(t)))
    else:
        check(lib().svtgpu_tile_plan_crop(width, height, int(crop[0]), int(crop[1]), ptr(us), sb, gx, gy, rank,
                                          ctypes.byref(t)))
    return t


_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t)


class _HostTransport(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allreduce_u64", _ALLREDUCE_FN)]


class Comm:
    """SvtGpuComm: the ranks of a picture tiled over GPUs.  Comm.rccl: RCCL over xGMI (one rank per device; rank 0
    makes the id with unique_id(), the caller broadcasts it); Comm.host: a host transport, `fn(words)` summing a uint64
    numpy array over the ranks in place (e.g. a gloo all_reduce) — several ranks on one GPU, CPU rehearsals.  Every
    exchange is bounded by `timeout_ms` (a host transport bounds its own wait by it: `fn(words, timeout_ms)` when fn
    takes two arguments, raising on expiry); an expired exchange raises SvtGpuError naming it, and the communicator
    fails from then on (`failed`)."""

    def __init__(self, h, keep=None):
        self.h, self._keep = h, keep

    @staticmethod
    def unique_id():
        b = (ctypes.c_uint8 * 128)()
        check(lib().svtgpu_comm_unique_id(b))
        return bytes(b)

    @classmethod
    def rccl(cls, ctx, nranks, rank, uid, timeout_ms=0, slot=-1):
        """svtgpu_comm_create_bounded: the RCCL communicator, its init bounded by timeout_ms (0: the default
        deadline); a peer that never joins raises SvtGpuError naming "communicator init", the slot and the rank."""
        b = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        h = _P()
        check(lib().svtgpu_comm_create_bounded(ctx.h, nranks, rank, b, int(timeout_ms), int(slot), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def host(cls, nranks, rank, fn):
        import inspect
        two = len(inspect.signature(fn).parameters) >= 2
        box = []  # the Comm, for its deadline

        def cb(user, buf, n):
            try:
                a = np.ctypeslib.as_array(buf, shape=(n,))
                if two:
                    fn(a, box[0]().timeout_ms)
                else:
                    fn(a)
                return 0
            except Exception:  # reported through the library's return code
                import traceback
                traceback.print_exc()
                return -1
        f = _ALLREDUCE_FN(cb)
        t = _HostTransport(None, f)
        h = _P()
        check(lib().svtgpu_comm_create_host(nranks, rank, ctypes.byref(t), ctypes.byref(h)))
        c = cls(h, keep=(f, t))
        import weakref
        box.append(weakref.ref(c))  # no reference cycle through the callback
        return c

    @property
    def nranks(self):
        return lib().svtgpu_comm_nranks(self.h)

    @property
    def timeout_ms(self):
        return lib().svtgpu_comm_timeout_ms(self.h)

    def set_timeout(self, ms):
        check(lib().svtgpu_comm_set_timeout(self.h, int(ms)))

    def set_slot(self, slot):
        check(lib().svtgpu_comm_set_slot(self.h, int(slot)))

    @property
    def failed(self):
        return bool(lib().svtgpu_comm_failed(self.h))

    def sync(self, stream=None):
        """Wait for `stream`, bounded by the deadline while a device-side exchange is outstanding."""
        check(lib().svtgpu_comm_sync(self.h, stream))

    def allreduce(self, words, stream=None):
        """Sum a host uint64 array over the ranks in place."""
        a = np.ascontiguousarray(words, np.uint64)
        check(lib().svtgpu_comm_allreduce_u64(self.h, ptr(a), a.size, 0, stream))
        return a

    def allreduce_device(self, dev_ptr, n, stream=None):
        """Sum n uint64 words of device memory over the ranks in place (enqueued on `stream`)."""
        check(lib().svtgpu_comm_allreduce_u64(self.h, ctypes.c_void_p(dev_ptr), n, 1, stream))

    def close(self):
        if self.h:
            lib().svtgpu_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rect(r):
    return None if r is None else (_I32 * 4)(*[int(x) for x in r])


def _rects3(r):
    return None if r is None else ((_I32 * 4) * 3)(*[(_I32 * 4)(*[int(x) for x in q]) for q in r])


class CdefState:
    """Device search state of one frame (mse_seg / skip_cdef_seg / cdef_dir_data)."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        h = _P()
        check(lib().svtgpu_cdef_state_create(ctx.h, width, height, ctypes.byref(h)))
        self.h = h
        self.nfb = lib().svtgpu_cdef_state_nfb(h)

    def set_block_mask(self, mask, stream=None):
        if mask is None:
            check(lib().svtgpu_cdef_set_block_mask(self.h, None, stream))
        else:
            self._mask = np.ascontiguousarray(mask, dtype=np.uint8)
            check(lib().svtgpu_cdef_set_block_mask(self.h, ptr(self._mask), stream))

    def set_fb_bsize(self, fb_bsize, stream=None):
        """SB128 mode info: BlockSize at each 64x64 filter block's top-left (None = SB64)."""
        if fb_bsize is None:
            check(lib().svtgpu_cdef_set_fb_bsize(self.h, None, stream))
        else:
            self._fbb = np.ascontiguousarray(fb_bsize, dtype=np.uint8)
            assert self._fbb.size == self.nfb
            check(lib().svtgpu_cdef_set_fb_bsize(self.h, ptr(self._fbb), stream))

    def search(self, recon, source, ctrls, base_q_idx, stream=None):
        check(lib().svtgpu_cdef_search_frame(self.h, recon.h, source.h, ctypes.byref(ctrls), base_q_idx, stream))

    def pick(self, ctrls, base_q_idx, lam, stream=None):
        prm = CdefParams()
        fbs = np.zeros(self.nfb, dtype=np.int8)
        check(lib().svtgpu_cdef_pick(self.h, ctypes.byref(ctrls), base_q_idx, lam, ctypes.byref(prm), ptr(fbs), stream))
        return prm, fbs

    def pick_async(self, ctrls, base_q_idx, lam, stream=None):
        """svtgpu_cdef_pick_async: the pick in stream order, no host wait; apply(params=None) uses its result."""
        check(lib().svtgpu_cdef_pick_async(self.h, ctypes.byref(ctrls), base_q_idx, lam, stream))

    def read_params(self, stream=None):
        """The last pick_async's parameters and per-FB strength indices (waits for `stream`)."""
        prm = CdefParams()
        fbs = np.zeros(self.nfb, dtype=np.int8)
        check(lib().svtgpu_cdef_read_params(self.h, ctypes.byref(prm), ptr(fbs), stream))
        return prm, fbs

    def set_fb_strength(self, fbs, stream=None):
        self._fbs = np.ascontiguousarray(fbs, dtype=np.int8)
        check(lib().svtgpu_cdef_set_fb_strength(self.h, ptr(self._fbs), stream))

    def apply(self, recon, out, params, stream=None):
        """params None: the last pick_async's parameters, from device memory."""
        check(lib().svtgpu_cdef_apply_frame(self.h, recon.h, out.h, ctypes.byref(params) if params is not None else None,
                                            stream))

    def read(self, stream=None):
        mse = np.empty((2, self.nfb, 64), dtype=np.uint64)
        skip = np.empty(self.nfb, dtype=np.uint8)
        d = np.empty((self.nfb, 64), dtype=np.uint8)
        v = np.empty((self.nfb, 64), dtype=np.int32)
        check(lib().svtgpu_cdef_read_state(self.h, ptr(mse), ptr(skip), ptr(d), ptr(v), stream))
        return mse, skip, d, v

    def set_fb_rows(self, begin, end):
        check(lib().svtgpu_cdef_set_fb_rows(self.h, begin, end))

    def set_tile(self, fb_rect=None, out_rect=None, comm=None):
        """svtgpu_cdef_set_tile: search fb_rect, pick over the tables summed over `comm`, apply into out_rect."""
        check(lib().svtgpu_cdef_set_tile(self.h, _rect(fb_rect), _rect(out_rect), comm.h if comm else None))

    def bind_tables(self, mse_dev_ptr, skip_dev_ptr):
        check(lib().svtgpu_cdef_bind_tables(self.h, mse_dev_ptr, skip_dev_ptr))

    def bind_dir_tables(self, dir_dev_ptr, var_dev_ptr):
        check(lib().svtgpu_cdef_bind_dir_tables(self.h, dir_dev_ptr, var_dev_ptr))

    def clear_tables(self, stream=None):
        check(lib().svtgpu_cdef_clear_tables(self.h, stream))

    def mse_device_ptr(self):
        return lib().svtgpu_cdef_mse_device_ptr(self.h)

    def close(self):
        if self.h:
            lib().svtgpu_cdef_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DlfState:
    """Deblocking state of one picture size: the device mode-info grid and the level tables."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        self.mi_rows, self.mi_cols = ((height + 7) & ~7) >> 2, ((width + 7) & ~7) >> 2
        h = _P()
        check(lib().svtgpu_dlf_state_create(ctx.h, width, height, ctypes.byref(h)))
        self.h = h

    def set_mode_info(self, mi, stream=None):
        """mi: structured array (LF_MI_DTYPE) or uint8 [mi_rows, mi_cols, 8]."""
        a = np.ascontiguousarray(mi)
        if a.dtype != LF_MI_DTYPE:
            a = np.ascontiguousarray(a.astype(np.uint8).reshape(self.mi_rows, self.mi_cols, 8))
        assert a.nbytes == self.mi_rows * self.mi_cols * 8, (a.shape, self.mi_rows, self.mi_cols)
        check(lib().svtgpu_dlf_set_mode_info(self.h, ptr(a), stream))  # staged: `mi` is free on return

    def set_mode_info_device(self, d_mi, stream=None):
        """The grid from device memory: a CUDA tensor of mi_rows * mi_cols * 8 bytes (or its address)."""
        if hasattr(d_mi, "data_ptr"):
            assert d_mi.is_cuda and d_mi.is_contiguous() and d_mi.numel() * d_mi.element_size() == \
                self.mi_rows * self.mi_cols * 8, (d_mi.shape, self.mi_rows, self.mi_cols)
            d_mi = d_mi.data_ptr()
        check(lib().svtgpu_dlf_set_mode_info_device(self.h, _P(d_mi), stream))

    def filter(self, frame, params, plane_start=0, plane_end=3, stream=None):
        """svtgpu_dlf_frame; params None: the levels of the last pick_async (on the device, in stream order)."""
        check(lib().svtgpu_dlf_frame(self.h, frame.h, None if params is None else ctypes.byref(params), plane_start,
                                     plane_end, stream))

    def filter_to(self, src, out, params, plane_start=0, plane_end=3, stream=None):
        """svtgpu_dlf_frame_to; params None: the levels of the last pick_async (on the device, in stream order)."""
        check(lib().svtgpu_dlf_frame_to(self.h, src.h, out.h, None if params is None else ctypes.byref(params),
                                        plane_start, plane_end, stream))

    def pick_async(self, recon, source, params, dlf_avg=0, dlf_avg_uv=0, temporal_layer_index=0, early_exit=2,
                   only_4x4=0, stream=None):
        """svtgpu_dlf_pick_async: the level search on the device, no host wait; filter(_to)(..., None) applies the
        picked levels, read_levels() returns them."""
        p = LfParams()
        ctypes.pointer(p)[0] = params
        check(lib().svtgpu_dlf_pick_async(self.h, recon.h, source.h, ctypes.byref(p), dlf_avg, dlf_avg_uv,
                                          temporal_layer_index, early_exit, only_4x4, stream))

    def async_rounds(self):
        """svtgpu_dlf_async_rounds: (rounds the last collected asynchronous search took, rounds enqueued)."""
        t, e = _I32(), _I32()
        check(lib().svtgpu_dlf_async_rounds(self.h, ctypes.byref(t), ctypes.byref(e)))
        return t.value, e.value

    def read_levels(self, stream=None):
        """svtgpu_dlf_read_levels: waits for the last pick_async and returns its LfParams."""
        p = LfParams()
        check(lib().svtgpu_dlf_read_levels(self.h, ctypes.byref(p), stream))
        return p

    def set_crop(self, crop_width, crop_height):
        """svtgpu_dlf_set_crop: no edge at or past the unpadded size is filtered (next set_mode_info on)."""
        check(lib().svtgpu_dlf_set_crop(self.h, crop_width, crop_height))

    def set_tile(self, sse_rect=None, out_rect=None, comm=None):
        """svtgpu_dlf_set_tile: trial SSEs over sse_rect summed over `comm`; the filter writes out_rect."""
        check(lib().svtgpu_dlf_set_tile(self.h, _rect(sse_rect), _rect(out_rect), comm.h if comm else None))

    def pick(self, recon, source, params, dlf_avg=0, dlf_avg_uv=0, temporal_layer_index=0, early_exit=2,
             only_4x4=0, stream=None):
        """Level search; `params` carries the previous levels in; returns the picked LfParams."""
        p = LfParams()
        ctypes.pointer(p)[0] = params
        check(lib().svtgpu_dlf_pick(self.h, recon.h, source.h, ctypes.byref(p), dlf_avg, dlf_avg_uv,
                                    temporal_layer_index, early_exit, only_4x4, stream))
        return p

    def close(self):
        if self.h:
            lib().svtgpu_dlf_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeBatch:
    """Open-loop full-pel ME (svtgpu_me_search): every 64x64 block x reference over a search area; per (block,
    reference) the 85 best SADs / MVs in the reference's Z-order numbering (64 8x8, 16 16x16, 4 32x32, 1 64x64)."""

    def __init__(self, ctx, width, height, nref):
        self.ctx, self.width, self.height, self.nref = ctx, width, height, nref
        h = _P()
        check(lib().svtgpu_me_batch_create(ctx.h, width, height, nref, ctypes.byref(h)))
        self.h = h
        self.nsb = ((width + 63) // 64) * ((height + 63) // 64)

    def set_origins(self, origin, stream=None):
        a = np.ascontiguousarray(origin, dtype=np.int16)
        assert a.shape == (self.nsb, self.nref, 2), a.shape
        check(lib().svtgpu_me_set_origins(self.h, ptr(a), stream))

    def search(self, source, refs, saw, sah, sub=0, sb_begin=0, sb_end=None, stream=None):
        assert len(refs) == self.nref
        arr = (_P * self.nref)(*[r.h for r in refs])
        end = self.nsb if sb_end is None else sb_end
        check(lib().svtgpu_me_search(self.h, source.h, arr, saw, sah, int(sub), sb_begin, end, stream))

    def read(self, sb_begin=0, sb_end=None, stream=None):
        end = self.nsb if sb_end is None else sb_end
        sad = np.empty((end - sb_begin, self.nref, 85), np.uint32)
        mv = np.empty((end - sb_begin, self.nref, 85), np.uint32)
        check(lib().svtgpu_me_read(self.h, ptr(sad), ptr(mv), sb_begin, end, stream))
        return sad, mv

    def close(self):
        if self.h:
            lib().svtgpu_me_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ObmcItem(ctypes.Structure):
    """SvtGpuObmcItem: one call of svt_av1_obmc_full_pixel_search."""
    FIELDS = ["ref", "x", "y", "w", "h", "mvp_col", "mvp_row", "ref_mv_col", "ref_mv_row", "col_min", "col_max",
              "row_min", "row_max", "sad_per_bit", "search_range", "search_diag", "cost_mode", "wm_offset",
              "cost_offset"]
    _fields_ = [(n, ctypes.c_int32) for n in FIELDS]


OBMC_RESULT_DTYPE = np.dtype([("mv_col", np.int32), ("mv_row", np.int32), ("best_sad", np.uint32),
                              ("variance", np.uint32), ("sse", np.uint32), ("steps", np.int32)])


class ObmcBatch:
    """Batched full-pel OBMC refinement (svtgpu_obmc_search): one item = one block's walk from its start MV; per item
    the final MV, the best SAD + cost, the OBMC variance / sse there and the moves made."""

    def __init__(self, ctx, width, height, nref, max_items):
        self.ctx, self.width, self.height, self.nref, self.max_items = ctx, width, height, nref, max_items
        h = _P()
        check(lib().svtgpu_obmc_batch_create(ctx.h, width, height, nref, max_items, ctypes.byref(h)))
        self.h = h
        self.nitems = 0

    def set_items(self, items, wm_pool, cost_pool=None, stream=None):
        """items: dicts (or ObmcItem) with the SvtGpuObmcItem fields; wm_pool / cost_pool: int32 arrays."""
        arr = (ObmcItem * max(len(items), 1))()
        for i, it in enumerate(items):
            arr[i] = it if isinstance(it, ObmcItem) else ObmcItem(**{k: int(it[k]) for k in ObmcItem.FIELDS})
        wm = np.ascontiguousarray(wm_pool, dtype=np.int32)
        cp = np.ascontiguousarray(cost_pool if cost_pool is not None else np.zeros(0), dtype=np.int32)
        self.nitems = 0
        check(lib().svtgpu_obmc_set_items(self.h, arr, len(items), ptr(wm), wm.size, ptr(cp) if cp.size else None,
                                          cp.size, stream))
        self.nitems = len(items)

    def set_items_device_wm(self, items, wm_count, cost_pool=None, stream=None):
        """svtgpu_obmc_set_items_device_wm: as set_items without a pool; returns the device address of the batch's pool of
        wm_count int32 entries, for TfState.obmc_weighted_src_batch to fill."""
        arr = (ObmcItem * max(len(items), 1))()
        for i, it in enumerate(items):
            arr[i] = it if isinstance(it, ObmcItem) else ObmcItem(**{k: int(it[k]) for k in ObmcItem.FIELDS})
        cp = np.ascontiguousarray(cost_pool if cost_pool is not None else np.zeros(0), dtype=np.int32)
        self.nitems = 0
        wm = _P()
        check(lib().svtgpu_obmc_set_items_device_wm(self.h, arr, len(items), int(wm_count), ptr(cp) if cp.size else None, cp.size,
                                                    ctypes.byref(wm), stream))
        self.nitems = len(items)
        return wm.value

    def search(self, refs, item_begin=0, item_end=None, stream=None):
        assert len(refs) == self.nref
        arr = (_P * self.nref)(*[r.h for r in refs])
        end = self.nitems if item_end is None else item_end
        check(lib().svtgpu_obmc_search(self.h, arr, item_begin, end, stream))

    def read(self, item_begin=0, item_end=None, stream=None):
        end = self.nitems if item_end is None else item_end
        out = np.zeros(max(end - item_begin, 0), OBMC_RESULT_DTYPE)
        check(lib().svtgpu_obmc_read(self.h, ptr(out), item_begin, end, stream))
        return out

    def close(self):
        if self.h:
            lib().svtgpu_obmc_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MdBatch:
    """Batched MD distortion: every SB x reference x AV1 block shape (SAD, sse, variance)."""

    def __init__(self, ctx, width, height, nref):
        self.ctx, self.width, self.height, self.nref = ctx, width, height, nref
        h = _P()
        check(lib().svtgpu_md_batch_create(ctx.h, width, height, nref, ctypes.byref(h)))
        self.h = h
        self.nsb = lib().svtgpu_md_batch_nsb(h)

    def set_mvs(self, mv, stream=None):
        a = np.ascontiguousarray(mv, dtype=np.int16)
        assert a.shape == (self.nsb, self.nref, 2), a.shape
        check(lib().svtgpu_md_set_mvs(self.h, ptr(a), stream))

    def run(self, source, refs, sb_begin=0, sb_end=None, stream=None):
        assert len(refs) == self.nref
        arr = (_P * self.nref)(*[r.h for r in refs])
        end = self.nsb if sb_end is None else sb_end
        check(lib().svtgpu_md_dist_batch(self.h, source.h, arr, sb_begin, end, stream))

    def read(self, sb_begin=0, sb_end=None, stream=None):
        end = self.nsb if sb_end is None else sb_end
        out = np.empty((end - sb_begin, self.nref, 3, MD_BLOCKS), np.uint32)
        check(lib().svtgpu_md_read(self.h, ptr(out), sb_begin, end, stream))
        return out

    def expand(self, sb_begin=0, sb_end=None, stream=None):
        """svtgpu_md_expand: every shape's values of the SB range from the cell moments (in stream order)."""
        end = self.nsb if sb_end is None else sb_end
        check(lib().svtgpu_md_expand(self.h, sb_begin, end, stream))

    def out_device_ptr(self):
        return lib().svtgpu_md_out_device_ptr(self.h)

    def close(self):
        if self.h:
            lib().svtgpu_md_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def md_layout():
    w, h, o = (np.zeros(19, np.int32) for _ in range(3))
    lib().svtgpu_md_layout(ptr(w), ptr(h), ptr(o))
    return w, h, o


class LrState:
    """Loop-restoration state of one picture size: unit grid and per-unit parameters per plane."""

    def __init__(self, ctx, width, height, unit_size):
        self.ctx, self.width, self.height = ctx, width, height
        self.unit_size = list(unit_size)
        us = np.ascontiguousarray(unit_size, np.int32)
        h = _P()
        check(lib().svtgpu_lr_state_create(ctx.h, width, height, ptr(us), ctypes.byref(h)))
        self.h = h
        self.units = []
        for p in range(3):
            hu, vu = _I32(), _I32()
            check(lib().svtgpu_lr_units(h, p, ctypes.byref(hu), ctypes.byref(vu)))
            self.units.append((hu.value, vu.value))

    def set_units(self, plane, units, stream=None):
        u = np.ascontiguousarray(units, REST_UNIT_DTYPE)
        assert len(u) == self.units[plane][0] * self.units[plane][1], (len(u), self.units[plane])
        check(lib().svtgpu_lr_set_units(self.h, plane, ptr(u), stream))

    def search(self, recon, source, ctrls, stream=None, records=False):
        """svtgpu_lr_search_frame: picks frame types and unit parameters (kept on the device for apply).
        Returns the frame types and, with records=True, the per-unit search records."""
        ft = np.zeros(3, np.int32)
        recs = [np.zeros(hu * vu, LR_UNIT_SEARCH_DTYPE) for hu, vu in self.units] if records else None
        rp = (ctypes.c_void_p * 3)(*[r.ctypes.data for r in recs]) if records else None
        check(lib().svtgpu_lr_search_frame(self.h, recon.h, source.h, ctypes.byref(ctrls), ptr(ft), rp, stream))
        return ([int(x) for x in ft], recs) if records else [int(x) for x in ft]

    def search_async(self, recon, source, ctrls, stream=None):
        """svtgpu_lr_search_frame_async: search + device RD finish enqueued on `stream`, no host wait; apply(...,
        frame_type=None) applies the result in stream order, read_result() collects the frame types."""
        check(lib().svtgpu_lr_search_frame_async(self.h, recon.h, source.h, ctypes.byref(ctrls), stream))

    def read_units(self, plane, stream=None):
        """svtgpu_lr_read_units: the state's units of `plane` (waits for an asynchronous search)."""
        u = np.zeros(self.units[plane][0] * self.units[plane][1], REST_UNIT_DTYPE)
        check(lib().svtgpu_lr_read_units(self.h, plane, ptr(u), stream))
        return u

    def read_sgr_planes(self, plane, slot, stream=None):
        """svtgpu_lr_read_sgr_planes: (ep, flt0, flt1) of ep slot `slot` of `plane` after a search: the int16 planes
        g = flt - (dgd << 4) of the r = 2 and r = 1 pass (None for a pass the ep does not have)."""
        w = (self.width + 1) >> 1 if plane else self.width
        h = (self.height + 1) >> 1 if plane else self.height
        f0, f1, ep = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16), _I32()
        check(lib().svtgpu_lr_read_sgr_planes(self.h, plane, slot, ctypes.byref(ep), ptr(f0), ptr(f1), stream))
        r0, r1 = SGR_RADII[ep.value]
        return ep.value, f0 if r0 else None, f1 if r1 else None

    def read_result(self, stream=None):
        """svtgpu_lr_read_result: waits for the last asynchronous search and returns its frame types."""
        ft = np.zeros(3, np.int32)
        check(lib().svtgpu_lr_read_result(self.h, ptr(ft), stream))
        return [int(x) for x in ft]

    def search_units(self, recon, source, ctrls, row_begin, row_end, records=None, stream=None):
        """svtgpu_lr_search_units: per-unit records of the unit rows [row_begin[p], row_end[p]) of every plane,
        written into `records` (per-plane arrays of all units; allocated zeroed when None).  No RD finish."""
        if records is None:
            records = [np.zeros(hu * vu, LR_UNIT_SEARCH_DTYPE) for hu, vu in self.units]
        rb = np.ascontiguousarray(row_begin, np.int32)
        re_ = np.ascontiguousarray(row_end, np.int32)
        rp = (ctypes.c_void_p * 3)(*[r.ctypes.data for r in records])
        check(lib().svtgpu_lr_search_units(self.h, recon.h, source.h, ctypes.byref(ctrls), ptr(rb), ptr(re_), rp,
                                           stream))
        return records

    PROFILE_CLASSES = ("stats", "sgr_filters", "wiener_trials", "projection", "other", "sgr_moments")

    def profile(self, enable=True, events=False, serial=False):
        """svtgpu_lr_profile: device-clock timing of the searches (enable: True = every class, a class name or a
        list of names = those classes, False = off).  Returns the per-class {launches, ms (device clock), ms_events
        (HIP events around each launch), bytes} totals of the
        searches timed since the previous call (kernel classes of svtgpu.h; untimed classes read 0) plus
        "searches", their count; reading synchronizes the device."""
        if enable is True:
            mask = -1
        elif not enable:
            mask = 0
        else:
            names = [enable] if isinstance(enable, str) else list(enable)
            mask = sum(1 << self.PROFILE_CLASSES.index(c) for c in names)
        if mask and events:
            mask = (63 if mask < 0 else mask) | 64
        if serial:  # both LR chains on one stream: each kernel's duration is its own (measurement)
            mask = (63 if mask < 0 else mask) | 128
        raw = np.zeros(1, LR_PROFILE_DTYPE)
        check(lib().svtgpu_lr_profile(self.h, mask, ptr(raw)))
        out = {c: {"launches": int(raw["launches"][0][i]), "ms": float(raw["ms"][0][i]),
                   "ms_events": float(raw["ms_events"][0][i]), "bytes": float(raw["bytes"][0][i])}
               for i, c in enumerate(self.PROFILE_CLASSES)}
        out["searches"] = int(raw["searches"][0])
        return out

    def set_tile(self, units=None, out=None, comm=None):
        """svtgpu_lr_set_tile: search units[p], records summed over `comm`, finish everywhere, apply into out[p]."""
        check(lib().svtgpu_lr_set_tile(self.h, _rects3(units), _rects3(out), comm.h if comm else None))

    def apply(self, deblocked, cdef_out, out, frame_type, stream=None):
        """svtgpu_lr_apply_frame; frame_type None: the units the last (asynchronous) search left on the device."""
        ft = None if frame_type is None else np.ascontiguousarray(frame_type, np.int32)
        check(lib().svtgpu_lr_apply_frame(self.h, deblocked.h, cdef_out.h, out.h, None if ft is None else ptr(ft),
                                          stream))

    def close(self):
        if self.h:
            lib().svtgpu_lr_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# radii (r = 2 pass, r = 1 pass) of the 16 self-guided parameter sets (svt_aom_eb_sgr_params)
SGR_RADII = [(2, 1)] * 10 + [(0, 1)] * 4 + [(2, 0)] * 2


def lr_controls(wn_level, sg_level, rdmult=0, switchable=(0, 0, 0), wiener=(0, 0), sgrproj=(0, 0)):
    """SvtGpuLrSearchControls of the reference's wn/sg filter levels plus the encoder's rate inputs."""
    c = LrSearchControls()
    check(lib().svtgpu_lr_controls_for_level(wn_level, sg_level, ctypes.byref(c)))
    c.rdmult = rdmult
    for i, v in enumerate(switchable):
        c.switchable_restore_cost[i] = v
    for i, v in enumerate(wiener):
        c.wiener_restore_cost[i] = v
    for i, v in enumerate(sgrproj):
        c.sgrproj_restore_cost[i] = v
    return c


def lr_finish_plane(ctrls, plane, records):
    """svtgpu_lr_finish_plane (host only): (frame restoration type, units) of a plane from all its records."""
    r = np.ascontiguousarray(records, LR_UNIT_SEARCH_DTYPE)
    units = np.zeros(len(r), REST_UNIT_DTYPE)
    ft = _I32()
    check(lib().svtgpu_lr_finish_plane(ctypes.byref(ctrls), plane, len(r), ptr(r), ctypes.byref(ft), ptr(units)))
    return ft.value, units


def lr_finish_frame(ctrls, records):
    """svtgpu_lr_finish_frame (host only): rest_finish_search of the whole frame over one RestUnitSearchInfo array
    shared by the planes.  records: per-plane arrays of all units.  Returns (frame types [3], units [3])."""
    rs = [np.ascontiguousarray(r, LR_UNIT_SEARCH_DTYPE) for r in records]
    units = [np.zeros(len(r), REST_UNIT_DTYPE) for r in rs]
    n = np.array([len(r) for r in rs], np.int32)
    ft = np.zeros(3, np.int32)
    rp = (ctypes.c_void_p * 3)(*[r.ctypes.data for r in rs])
    up = (ctypes.c_void_p * 3)(*[u.ctypes.data for u in units])
    check(lib().svtgpu_lr_finish_frame(ctypes.byref(ctrls), ptr(n), rp, ptr(ft), up))
    return [int(x) for x in ft], units


# ---------------------------------------------------------------------------------------------
# multi-GPU decomposition (one rank per GPU): balanced bands of rows; the only data-path exchanges are
# the CDEF mse/skip table all-reduce and the LR record all-gather
# ---------------------------------------------------------------------------------------------
def band(count, n, rank):
    """[begin, end) of `rank`'s share of `count` rows split into `n` balanced contiguous bands."""
    edges = np.linspace(0, count, n + 1).round().astype(int)
    return int(edges[rank]), int(edges[rank + 1])


def lr_unit_rows(units, n, rank):
    """Per-plane unit-row bands (row_begin[3], row_end[3]) of `rank` for an LrState.units list [(hu, vu)]."""
    rb, re_ = zip(*(band(vu, n, rank) for _, vu in units))
    return list(rb), list(re_)


def gather_lr_records(records, units, n, rank, group=None, device=None):
    """All-gather the per-unit LR search records of every rank's unit-row band (torch.distributed; RCCL with
    device="cuda", gloo with device=None).  `records`: per-plane arrays of all units with this rank's band
    filled.  Returns the merged per-plane arrays (every unit from the rank that searched it)."""
    import torch
    import torch.distributed as dist
    merged = []
    for p, (hu, vu) in enumerate(units):
        raw = torch.from_numpy(np.ascontiguousarray(records[p]).view(np.uint8).copy())
        if device is not None:
            raw = raw.to(device)
        parts = [torch.empty_like(raw) for _ in range(n)]
        dist.all_gather(parts, raw, group=group)
        out = np.zeros(hu * vu, LR_UNIT_SEARCH_DTYPE)
        for r in range(n):
            b, e = band(vu, n, r)
            got = parts[r].cpu().numpy().view(LR_UNIT_SEARCH_DTYPE)
            out[b * hu:e * hu] = got[b * hu:e * hu]
        merged.append(out)
    return merged


class CcsoState:
    """CCSO on the device: the reference's ccso_search / derive_ccso_filter and ccso_frame
    (EbPickccso.c:464-815, EbCcso.c:626-678) over device buffers given as integer addresses (e.g. a torch tensor's
    data_ptr()).  org / rec / the planes' samples use the luma width as stride (ccso_stride)."""

    def __init__(self, ctx, width, height):
        self.ctx, self.width, self.height = ctx, width, height
        h = _P()
        check(lib().svtgpu_ccso_state_create(ctx.h, width, height, ctypes.byref(h)))
        self.h = h

    def grid(self, plane):
        a, b = _I32(), _I32()
        check(lib().svtgpu_ccso_grid(self.width, self.height, plane, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def extend(self, luma, bits, stride, ext, stream=None):
        """ext_rec_y (EbPickccso.c:907-918 + extend_ccso_border) from a device luma plane into `ext`."""
        check(lib().svtgpu_ccso_extend_luma(luma, bits, stride, self.width, self.height, ext, stream))

    def search_plane(self, ext, org, rec, plane, bit_depth, rdmult, stream=None, read=True):
        """derive_ccso_filter of one plane; (CcsoParams, flags (nvfb, nhfb) uint8) when read, else None (the result
        stays on the device for apply(params=None))."""
        if not read:
            check(lib().svtgpu_ccso_search_plane(self.h, ext, org, rec, plane, bit_depth, rdmult, None, None, stream))
            return None
        prm, flags = CcsoParams(), np.zeros(self.grid(plane), np.uint8)
        check(lib().svtgpu_ccso_search_plane(self.h, ext, org, rec, plane, bit_depth, rdmult, ctypes.byref(prm),
                                             ptr(flags), stream))
        return prm, flags

    def search_frame(self, ext, org, rec, bit_depth, rdmult, base_q_idx, stream=None, read=True):
        """ccso_search: (rc, [CcsoParams] * 3, [flags] * 3, frame_flag); rc 1 = rdmult overflow, nothing searched.
        read=False: no read-back and no host wait (rc only); the results stay on the device for apply()."""
        if not read:
            rc = lib().svtgpu_ccso_search_frame(self.h, ext, (_P * 3)(*org), (_P * 3)(*rec), bit_depth, rdmult,
                                                base_q_idx, None, None, ctypes.byref(_I32(0)), stream)
            if rc not in (0, 1):
                check(rc)
            return rc
        prms = (CcsoParams * 3)()
        flags = [np.zeros(self.grid(p), np.uint8) for p in range(3)]
        ff = _I32(0)
        rc = lib().svtgpu_ccso_search_frame(self.h, ext, (_P * 3)(*org), (_P * 3)(*rec), bit_depth, rdmult,
                                            base_q_idx, prms, (_P * 3)(*[f.ctypes.data for f in flags]),
                                            ctypes.byref(ff), stream)
        if rc not in (0, 1):
            check(rc)
        return rc, list(prms), flags, ff.value

    def apply(self, ext, plane, bit_depth, dst, dst_bits, dst_stride, params=None, flags=None, stream=None):
        """ccso_frame's body for one plane, in place on the device plane `dst`; params None: the last search's."""
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        check(lib().svtgpu_ccso_apply_plane(self.h, ext, plane, bit_depth, dst, dst_bits, dst_stride,
                                            None if params is None else ctypes.byref(params), ptr(f), stream))

    def close(self):
        if self.h:
            lib().svtgpu_ccso_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plane_sse(a, b, plane, stream=None):
    v = _U64()
    check(lib().svtgpu_plane_sse(a.h, b.h, plane, ctypes.byref(v), stream))
    return v.value


def superres_scaled_size(dim, denom):
    """svtgpu_superres_scaled_size: the downscaled size of `dim` for a superres / resize denominator (host only)."""
    return int(lib().svtgpu_superres_scaled_size(int(dim), int(denom)))


def superres_geometry(in_w, out_w):
    """svtgpu_superres_geometry: (x_step_qn, x0_qn) of an upscale of in_w to out_w samples (host only)."""
    step, x0 = _I32(0), _I32(0)
    check(lib().svtgpu_superres_geometry(int(in_w), int(out_w), ctypes.byref(step), ctypes.byref(x0)))
    return int(step.value), int(x0.value)


def superres_upscale(src, dst, frame_width, upscaled_width, stream=None):
    """svtgpu_superres_upscale_frame: the normative upscale of the three planes of Frame `src` (crop width frame_width)
    into Frame `dst` (crop width upscaled_width), asynchronous on `stream`."""
    check(lib().svtgpu_superres_upscale_frame(src.h, dst.h, int(frame_width), int(upscaled_width), stream))


def resize_plan(in_length, out_length):
    """svtgpu_resize_plan: (halving steps, the length that reaches the interpolation, table index or -1, delta, offset)
    of one 1-D resize of in_length to out_length samples (host only)."""
    v = [_I32(0) for _ in range(4)]
    check(lib().svtgpu_resize_plan(int(in_length), int(out_length), *[ctypes.byref(x) for x in v]))
    n = int(in_length)
    for _ in range(v[0].value):
        n = (n + 1) >> 1
    return int(v[0].value), n, int(v[1].value), int(v[2].value), int(v[3].value)


def resize_filter(filter_index):
    """svtgpu_resize_filter: table 0..4 (0.5 / 0.625 / 0.75 / 0.875-band, normative) as int16 [64][8] (host only)."""
    a = np.zeros((64, 8), np.int16)
    check(lib().svtgpu_resize_filter(int(filter_index), ptr(a)))
    return a


def resize_half_filters():
    """svtgpu_resize_half_filters: the (symeven, symodd) half filters of the factor-of-2 steps (host only)."""
    e, o = np.zeros(4, np.int16), np.zeros(4, np.int16)
    check(lib().svtgpu_resize_half_filters(ptr(e), ptr(o)))
    return e, o


def resize(src, dst, src_w, src_h, dst_w, dst_h, stream=None):
    """svtgpu_resize_frame: the three planes of Frame `src` (crop size src_w x src_h) resized into Frame `dst` (crop size
    dst_w x dst_h) as svt_aom_resize_frame does, asynchronous on `stream`."""
    check(lib().svtgpu_resize_frame(src.h, dst.h, int(src_w), int(src_h), int(dst_w), int(dst_h), stream))


def tf_tables():
    """svtgpu_tf_tables: the library's (log1p_tab_fp16, sqrt_array_fp16, expf_tab_fp16) as numpy arrays (host only)."""
    l, q, e, nl, ne = _P(), _P(), _P(), _I32(0), _I32(0)
    check(lib().svtgpu_tf_tables(ctypes.byref(l), ctypes.byref(nl), ctypes.byref(q), ctypes.byref(e), ctypes.byref(ne)))
    return (np.ctypeslib.as_array(ctypes.cast(l, ctypes.POINTER(_I32)), (nl.value,)).copy(),
            np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_uint32)), (16,)).copy(),
            np.ctypeslib.as_array(ctypes.cast(e, ctypes.POINTER(_I32)), (ne.value,)).copy())


def tf_noise_log1p_fp16(noise_level_fp16):
    return int(lib().svtgpu_tf_noise_log1p_fp16(int(noise_level_fp16)))


def tf_decay_factor_fp16(decay_control, noise_log1p_fp16, q):
    return int(lib().svtgpu_tf_decay_factor_fp16(int(decay_control), int(noise_log1p_fp16), int(q)))


def tf_estimate_noise(ctx, plane_ptr, bits, stride, w, h, stream=None):
    """svtgpu_tf_estimate_noise of a device plane (synchronous)."""
    v = _I32(0)
    check(lib().svtgpu_tf_estimate_noise(ctx.h, plane_ptr, int(bits), int(stride), int(w), int(h), stream, ctypes.byref(v)))
    return int(v.value)


class TfState:
    """svtgpu_tf_state_*: the temporal filter's per-picture-size state (metadata on the device, the noise result slot)."""

    def __init__(self, ctx, width, height):
        h = _P()
        check(lib().svtgpu_tf_state_create(ctx.h, int(width), int(height), ctypes.byref(h)))
        self.h, self.ctx, self.width, self.height = h, ctx, int(width), int(height)
        self.nblk = ((self.width + 63) // 64) * ((self.height + 63) // 64)

    def close(self):
        if self.h:
            lib().svtgpu_tf_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate_noise_async(self, plane_ptr, bits, stride, w, h, stream=None):
        check(lib().svtgpu_tf_estimate_noise_async(self.h, plane_ptr, int(bits), int(stride), int(w), int(h), stream))

    def read_noise(self, stream=None):
        v = _I32(0)
        check(lib().svtgpu_tf_read_noise(self.h, stream, ctypes.byref(v)))
        return int(v.value)

    def filter_frame(self, centre, refs, blocks, params, out, stream=None):
        """centre / out: TfPlanes; refs: a list of TfPlanes; blocks: a list of TfBlock, [reference][block] flattened."""
        n = len(refs)
        assert len(blocks) == n * self.nblk, "one TfBlock per (reference, 64x64 block)"
        ra = (TfPlanes * max(n, 1))(*refs)
        ba = (TfBlock * max(len(blocks), 1))(*blocks)
        check(lib().svtgpu_tf_filter_frame(self.h, ctypes.byref(centre), ra if n else None, n, ba if n else None,
                                           ctypes.byref(params), ctypes.byref(out), stream))


    def predict_frame(self, refs, border_x, border_y, motion, bit_depth, tf_chroma, pred, stream=None):
        """refs / pred: lists of TfPlanes (refs at sample (0, 0) of the padded pictures); motion: a list of TfMotion,
        [reference][block] flattened."""
        n = len(refs)
        assert len(pred) == n and len(motion) == n * self.nblk, "one TfMotion per (reference, 64x64 block)"
        ra, pa = (TfPlanes * max(n, 1))(*refs), (TfPlanes * max(n, 1))(*pred)
        ma = (TfMotion * max(len(motion), 1))(*motion)
        check(lib().svtgpu_tf_predict_frame(self.h, ra if n else None, n, int(border_x), int(border_y), ma if n else None,
                                            int(bit_depth), int(tf_chroma), pa if n else None, stream))

    def compound_predict_batch(self, refs, border_x, border_y, blocks, bit_depth, chroma, pred, stream=None):
        """svtgpu_compound_predict_batch: refs a list of TfPlanes at sample (0, 0) of the padded pictures; blocks a list of
        CompoundBlock; pred one TfPlanes, the predictor picture."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (CompoundBlock * max(nb, 1))(*blocks)
        check(lib().svtgpu_compound_predict_batch(self.h, ra, n, int(border_x), int(border_y), ba, nb, int(bit_depth),
                                                  int(chroma), ctypes.byref(pred), stream))

    def masked_compound_predict_batch(self, refs, border_x, border_y, blocks, bit_depth, chroma, pred, stream=None):
        """svtgpu_masked_compound_predict_batch: as compound_predict_batch, on a list of MaskedCompoundBlock."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (MaskedCompoundBlock * max(nb, 1))(*blocks)
        check(lib().svtgpu_masked_compound_predict_batch(self.h, ra, n, int(border_x), int(border_y), ba, nb, int(bit_depth),
                                                         int(chroma), ctypes.byref(pred), stream))

    def warp_predict_batch(self, refs, blocks, bit_depth, chroma, pred, stream=None):
        """svtgpu_warp_predict_batch: refs a list of TfPlanes at sample (0, 0) of the reference pictures (no border is read);
        blocks a list of WarpBlock; pred one TfPlanes, the predictor picture."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (WarpBlock * max(nb, 1))(*blocks)
        check(lib().svtgpu_warp_predict_batch(self.h, ra, n, ba, nb, int(bit_depth), int(chroma), ctypes.byref(pred), stream))

    def obmc_predict_batch(self, refs, border_x, border_y, blocks, bit_depth, chroma, pred, stream=None):
        """svtgpu_obmc_predict_batch: refs a list of TfPlanes at sample (0, 0) of the padded pictures; blocks a list of
        ObmcBlock; pred one TfPlanes, the predictor picture."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (ObmcBlock * max(nb, 1))(*blocks)
        check(lib().svtgpu_obmc_predict_batch(self.h, ra, n, int(border_x), int(border_y), ba, nb, int(bit_depth), int(chroma),
                                              ctypes.byref(pred), stream))

    def obmc_weighted_src_batch(self, refs, border_x, border_y, src_luma, src_stride, blocks, wm_dev, wm_count, stream=None):
        """svtgpu_obmc_weighted_src_batch: src_luma / wm_dev device addresses; blocks a list of ObmcBlock with wm_offset set."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (ObmcBlock * max(nb, 1))(*blocks)
        check(lib().svtgpu_obmc_weighted_src_batch(self.h, ra, n, int(border_x), int(border_y), src_luma, int(src_stride), ba, nb,
                                                   wm_dev, int(wm_count), stream))

    def interintra_predict_batch(self, refs, border_x, border_y, blocks, edges, bit_depth, chroma, pred, stream=None):
        """svtgpu_interintra_predict_batch: refs a list of TfPlanes at sample (0, 0) of the padded pictures; blocks a list of
        InterIntraBlock; edges the edge pool, a 1-D numpy array of the picture's sample type (uint8 / uint16); pred one
        TfPlanes, the predictor picture."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (InterIntraBlock * max(nb, 1))(*blocks)
        assert edges.dtype == (np.uint16 if bit_depth > 8 else np.uint8) and edges.flags.c_contiguous
        check(lib().svtgpu_interintra_predict_batch(self.h, ra, n, int(border_x), int(border_y), ba, nb, edges.ctypes.data,
                                                    int(edges.size), int(bit_depth), int(chroma), ctypes.byref(pred), stream))

    def interintra_mode_sse_batch(self, refs, border_x, border_y, blocks, edges, bit_depth, src_luma, src_stride, sse_dev,
                                  stream=None):
        """svtgpu_interintra_mode_sse_batch: as interintra_predict_batch; src_luma / sse_dev device addresses (the source luma
        plane of the picture's sample type; 4 * len(blocks) int64)."""
        n, nb = len(refs), len(blocks)
        ra, ba = (TfPlanes * max(n, 1))(*refs), (InterIntraBlock * max(nb, 1))(*blocks)
        assert edges.dtype == (np.uint16 if bit_depth > 8 else np.uint8) and edges.flags.c_contiguous
        check(lib().svtgpu_interintra_mode_sse_batch(self.h, ra, n, int(border_x), int(border_y), ba, nb, edges.ctypes.data,
                                                     int(edges.size), int(bit_depth), src_luma, int(src_stride), sse_dev, stream))

    def search_frame(self, centre, refs, border_x, border_y, fullpel, params, stream=None):
        """centre: TfPlanes (luma read); refs: a list of TfPlanes at sample (0, 0) of the padded pictures; fullpel: a list
        of TfFullpel, [reference][block] flattened; params: TfSearchParams.  The records stay on the device."""
        n = len(refs)
        assert len(fullpel) == n * self.nblk, "one TfFullpel per (reference, 64x64 block)"
        ra = (TfPlanes * max(n, 1))(*refs)
        fa = (TfFullpel * max(len(fullpel), 1))(*fullpel)
        check(lib().svtgpu_tf_search_frame(self.h, ctypes.byref(centre), ra if n else None, n, int(border_x), int(border_y),
                                           fa if n else None, ctypes.byref(params), stream))

    def search_read(self, n_refs, stream=None):
        """The records of the last search: (a TfMotion array, a TfBlock array), [reference][block] flattened."""
        mo, bl = (TfMotion * (n_refs * self.nblk))(), (TfBlock * (n_refs * self.nblk))()
        check(lib().svtgpu_tf_search_read(self.h, int(n_refs), mo, bl, stream))
        return mo, bl

    def compensate_filter_frame(self, centre, refs, border_x, border_y, params, sub_sampling_shift, pred, out, stream=None):
        """The chain behind search_frame on the state's records: compensation into pred, err32 of the use64 blocks, the
        filter into out.  centre / out: TfPlanes; refs / pred: lists of TfPlanes; params: TfParams."""
        n = len(refs)
        assert len(pred) == n
        ra, pa = (TfPlanes * max(n, 1))(*refs), (TfPlanes * max(n, 1))(*pred)
        check(lib().svtgpu_tf_compensate_filter_frame(self.h, ctypes.byref(centre), ra if n else None, n, int(border_x),
                                                      int(border_y), ctypes.byref(params), int(sub_sampling_shift),
                                                      pa if n else None, ctypes.byref(out), stream))


def interp_tables():
    """svtgpu_interp_tables: the library's six sub-pel filter tables as an int16 array [6][16][8] (host only)."""
    t, n = _P(), _I32(0)
    check(lib().svtgpu_interp_tables(ctypes.byref(t), ctypes.byref(n)))
    return np.ctypeslib.as_array(ctypes.cast(t, _I16P), (n.value, 16, 8)).copy()


def convolve_sr(form, src, x0, y0, w, h, filter_x, filter_y, round_0, round_1, bd, dst, dx0, dy0):
    """One of the eight interpolation shims (form in INTERP_FORMS): the w x h block at (x0, y0) of the host array `src`
    (uint8 at bd 8, else uint16) into `dst` at (dx0, dy0), in place."""
    hbd = src.dtype == np.uint16
    fn = getattr(lib(), ("svtgpu_av1_highbd_convolve_" if hbd else "svtgpu_av1_convolve_") + form)
    fx = (ctypes.c_int16 * 8)(*[int(v) for v in filter_x])
    fy = (ctypes.c_int16 * 8)(*[int(v) for v in filter_y])
    sp = src.ctypes.data + (y0 * src.strides[0] + x0 * src.itemsize)
    dp = dst.ctypes.data + (dy0 * dst.strides[0] + dx0 * dst.itemsize)
    args = [sp, src.strides[0] // src.itemsize, dp, dst.strides[0] // dst.itemsize, int(w), int(h), fx, fy, int(round_0),
            int(round_1)]
    fn(*(args + [int(bd)] if hbd else args))


def dist_wtd_weights(d0, d1, order_idx):
    """svtgpu_dist_wtd_weights: (fwd_offset, bck_offset) of COMPOUND_DISTWTD from the two frame distances (host only)."""
    f, b = _I32(0), _I32(0)
    check(lib().svtgpu_dist_wtd_weights(int(d0), int(d1), int(order_idx), ctypes.byref(f), ctypes.byref(b)))
    return int(f.value), int(b.value)


def jnt_convolve(form, src, x0, y0, w, h, filter_x, filter_y, round_0, round_1, bd, conv_dst, do_average, dist_wtd=0,
                 fwd_offset=0, bck_offset=0, dst=None, dx0=0, dy0=0):
    """One of the eight compound shims (form in COMPOUND_FORMS): the w x h block at (x0, y0) of the host array `src`
    (uint8 at bd 8, else uint16) with the uint16 array `conv_dst` as ConvolveParams::dst (block at its (0, 0)); with
    do_average the pixels land in `dst` at (dx0, dy0), in place."""
    hbd = src.dtype == np.uint16
    fn = getattr(lib(), ("svtgpu_av1_highbd_jnt_convolve_" if hbd else "svtgpu_av1_jnt_convolve_") + form)
    fx = (ctypes.c_int16 * 8)(*[int(v) for v in filter_x])
    fy = (ctypes.c_int16 * 8)(*[int(v) for v in filter_y])
    assert conv_dst.dtype == np.uint16 and (dst is None or dst.dtype == src.dtype)
    sp = src.ctypes.data + (y0 * src.strides[0] + x0 * src.itemsize)
    dp = None if dst is None else dst.ctypes.data + (dy0 * dst.strides[0] + dx0 * dst.itemsize)
    args = [sp, src.strides[0] // src.itemsize, dp, 0 if dst is None else dst.strides[0] // dst.itemsize, int(w), int(h), fx,
            fy, int(round_0), int(round_1), conv_dst.ctypes.data, conv_dst.strides[0] // 2, int(do_average), int(dist_wtd),
            int(fwd_offset), int(bck_offset)]
    fn(*(args + [int(bd)] if hbd else args))


def wedge_mask(w, h, wedge_index, wedge_sign):
    """svtgpu_wedge_mask: the w x h wedge mask as a uint8 array [h][w] (host only)."""
    m = np.zeros((int(h), int(w)), np.uint8)
    check(lib().svtgpu_wedge_mask(int(w), int(h), int(wedge_index), int(wedge_sign), m.ctypes.data))
    return m


def diffwtd_mask(mask_type, src0, src1, w, h, round_0, round_1, bd):
    """svtgpu_av1_build_compound_diffwtd_mask_d16 on the top-left w x h of the uint16 arrays src0 / src1 (any strides): the
    packed uint8 mask [h][w]."""
    assert src0.dtype == np.uint16 and src1.dtype == np.uint16
    m = np.zeros((int(h), int(w)), np.uint8)
    lib().svtgpu_av1_build_compound_diffwtd_mask_d16(m.ctypes.data, int(mask_type), src0.ctypes.data, src0.strides[0] // 2,
                                                     src1.ctypes.data, src1.strides[0] // 2, int(h), int(w), int(round_0),
                                                     int(round_1), int(bd))
    return m


def blend_a64_d16_mask(dst, dx0, dy0, src0, src1, mask, w, h, subw, subh, round_0, round_1, bd):
    """svtgpu_aom_lowbd_blend_a64_d16_mask (dst uint8) or svtgpu_aom_highbd_blend_a64_d16_mask (dst uint16): the w x h block
    into `dst` at (dx0, dy0), in place, from the top-left corners of the uint16 arrays src0 / src1 and the uint8 mask."""
    assert src0.dtype == np.uint16 and src1.dtype == np.uint16 and mask.dtype == np.uint8
    dp = dst.ctypes.data + dy0 * dst.strides[0] + dx0 * dst.itemsize
    args = [dp, dst.strides[0] // dst.itemsize, src0.ctypes.data, src0.strides[0] // 2, src1.ctypes.data, src1.strides[0] // 2,
            mask.ctypes.data, mask.strides[0], int(w), int(h), int(subw), int(subh), int(round_0), int(round_1)]
    if dst.dtype == np.uint16:
        lib().svtgpu_aom_highbd_blend_a64_d16_mask(*(args + [int(bd)]))
    else:
        lib().svtgpu_aom_lowbd_blend_a64_d16_mask(*args)


def warp_filter_table():
    """svtgpu_warp_filter_table: the library's warped filter table as an int16 array [193][8] (host only)."""
    t, n = _P(), _I32(0)
    check(lib().svtgpu_warp_filter_table(ctypes.byref(t), ctypes.byref(n)))
    return np.ctypeslib.as_array(ctypes.cast(t, _I16P), (n.value, 8)).copy()


def blend_a64_mask(direction, dst, src0, src1, mask, w, h, bd=8, form=None):
    """One of the six OBMC blend shims on host arrays given as (array, x0, y0): direction "v" or "h"; form None (8-bit
    samples), "16bit", or "8bit" (16-bit samples behind a uint8_t *).  dst is written in place."""
    def at(v):
        a, x0, y0 = v
        ptr = a.ctypes.data + y0 * a.strides[0] + x0 * a.itemsize
        return ptr, a.strides[0] // a.itemsize
    m = (ctypes.c_uint8 * len(mask))(*[int(v) for v in mask])
    (dp, ds), (p0, s0), (p1, s1) = at(dst), at(src0), at(src1)
    name = "svtgpu_aom_blend_a64_%smask" % direction if form is None else "svtgpu_aom_highbd_blend_a64_%smask_%s" % (direction, form)
    args = [dp, ds, p0, s0, p1, s1, m, int(w), int(h)]
    getattr(lib(), name)(*(args if form is None else args + [int(bd)]))


def obmc_mask(length):
    """svtgpu_obmc_mask: the 1-D OBMC mask of `length` (1, 2, 4, 8, 16 or 32) as a list (host only)."""
    m = _P()
    check(lib().svtgpu_obmc_mask(int(length), ctypes.byref(m)))
    return list(ctypes.cast(m, ctypes.POINTER(ctypes.c_uint8))[:int(length)])


def interintra_smooth_mask(w, h, mode):
    """svtgpu_interintra_smooth_mask: the smooth inter-intra mask of `mode` for a w x h plane block as a uint8 array [h][w]
    (host only)."""
    m = np.zeros((int(h), int(w)), np.uint8)
    check(lib().svtgpu_interintra_smooth_mask(int(w), int(h), int(mode), m.ctypes.data))
    return m


def blend_a64_mask2d(dst, src0, src1, mask, w, h, subw, subh, bd=None):
    """svtgpu_aom_blend_a64_mask (bd None, uint8 arrays) or svtgpu_aom_highbd_blend_a64_mask (uint16 arrays) on host arrays
    given as (array, x0, y0); mask a uint8 array [h << subh][w << subw] (any row stride).  dst is written in place."""
    def at(v):
        a, x0, y0 = v
        return a.ctypes.data + y0 * a.strides[0] + x0 * a.itemsize, a.strides[0] // a.itemsize
    assert mask.dtype == np.uint8
    (dp, ds), (p0, s0), (p1, s1) = at(dst), at(src0), at(src1)
    args = [dp, ds, p0, s0, p1, s1, mask.ctypes.data, mask.strides[0], int(w), int(h), int(subw), int(subh)]
    if bd is None:
        lib().svtgpu_aom_blend_a64_mask(*args)
    else:
        lib().svtgpu_aom_highbd_blend_a64_mask(*(args + [int(bd)]))


def intra_predictor(kind, above, left, bd=None):
    """svtgpu_aom_intra_predictor (bd None, uint8) or svtgpu_aom_highbd_intra_predictor (uint16): the len(left) x len(above)
    block of `kind` (a name of INTRA_KINDS) as an array [h][w]."""
    hbd = bd is not None
    t = np.uint16 if hbd else np.uint8
    a, l = np.ascontiguousarray(above, t), np.ascontiguousarray(left, t)
    out = np.zeros((l.size, a.size), t)
    args = [out.ctypes.data, a.size, a.ctypes.data, l.ctypes.data, a.size, l.size, INTRA_KINDS.index(kind)]
    if hbd:
        lib().svtgpu_aom_highbd_intra_predictor(*(args + [int(bd)]))
    else:
        lib().svtgpu_aom_intra_predictor(*args)
    return out


def warp_shear_params(wmmat):
    """svtgpu_warp_shear_params: (the reference's return value 1 / 0, [alpha, beta, gamma, delta]) of six model values."""
    m, o = (ctypes.c_int32 * 6)(*[int(v) for v in wmmat]), (ctypes.c_int16 * 4)()
    rc = lib().svtgpu_warp_shear_params(m, o)
    if rc < 0:
        check(rc)
    return rc, [int(v) for v in o]


def warp_affine(mat, ref, ref2b, pred, px0, py0, p_col, p_row, p_width, p_height, ss_x, ss_y, bd, round_0, round_1, is_compound,
                conv_dst, do_average, dist_wtd, fwd_offset, bck_offset, abgd):
    """svtgpu_av1_warp_affine (ref2b None: ref a uint8 plane) or svtgpu_av1_highbd_warp_affine (ref the uint8 plane of the
    high bits, ref2b that of the low two): the p_width x p_height block into `pred` at (px0, py0) and / or the uint16 array
    `conv_dst` (block at its (0, 0)), in place.  Returns the shim's code."""
    m = (ctypes.c_int32 * 6)(*[int(v) for v in mat])
    pp = None if pred is None else pred.ctypes.data + py0 * pred.strides[0] + px0 * pred.itemsize
    ps = 0 if pred is None else pred.strides[0] // pred.itemsize
    cp = None if conv_dst is None else conv_dst.ctypes.data
    cs = 0 if conv_dst is None else conv_dst.strides[0] // 2
    tail = [int(round_0), int(round_1), int(is_compound), cp, cs, int(do_average), int(dist_wtd), int(fwd_offset), int(bck_offset)] + \
           [int(v) for v in abgd]
    h, w = ref.shape
    if ref2b is None:
        return lib().svtgpu_av1_warp_affine(m, ref.ctypes.data, w, h, ref.strides[0], pp, int(p_col), int(p_row), int(p_width),
                                            int(p_height), ps, int(ss_x), int(ss_y), *tail)
    return lib().svtgpu_av1_highbd_warp_affine(m, ref.ctypes.data, ref2b.ctypes.data, w, h, ref.strides[0], ref2b.strides[0], pp,
                                               int(p_col), int(p_row), int(p_width), int(p_height), ps, int(ss_x), int(ss_y),
                                               int(bd), *tail)


def declared_symbols(header=HEADER_PATH):
    """Function names declared in include/svtgpu.h (for the ABI export test)."""
    import re
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(svtgpu_[a-z0-9_]+)\s*\(", txt)))


def transfer_bytes(reset=False):
    """svtgpu_transfer_bytes: (host-to-device, device-to-host) bytes moved by the frame-level entry points since the
    last reset (copies and results read from mapped memory)."""
    h2d, d2h = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib().svtgpu_transfer_bytes(ctypes.byref(h2d), ctypes.byref(d2h), 1 if reset else 0))
    return int(h2d.value), int(d2h.value)
