"""ctypes binding of include/heifgpu.h (libheifgpu.so, built in-tree).

The product path has no CPU fallback: if the HIP library is missing this
module raises at import time.
"""
from __future__ import annotations

import ctypes
import os
import pathlib

_HERE = pathlib.Path(__file__).resolve().parent
# HEIFGPU_LIBRARY selects another in-tree build of the same ABI (e.g. the
# counter-instrumented heif_amd/libheifgpu_prof.so from `make prof`)
LIB_PATH = pathlib.Path(os.environ.get("HEIFGPU_LIBRARY", _HERE / "libheifgpu.so"))

HEIFGPU_OK = 0
HEIFGPU_E_INVALID = -1
HEIFGPU_E_PARSE = -2
HEIFGPU_E_UNSUPPORTED = -3
HEIFGPU_E_DEVICE = -4
HEIFGPU_E_DECODE = -5

STATUS_BITS = {
    1 << 0: "cabac_init",
    1 << 1: "substream_end",
    1 << 2: "overrun",
    1 << 3: "syntax",
    1 << 4: "unsupported",
    1 << 5: "capacity",
}


class ImageInfo(ctypes.Structure):
    _fields_ = [
        (name, ctypes.c_uint32)
        for name in (
            "width", "height", "chroma_format_idc", "bit_depth", "bytes_per_sample", "grid_rows",
            "grid_cols", "tile_width", "tile_height", "num_tiles", "rotation", "ispe_width",
            "ispe_height", "coded_bytes", "primary_item_id", "num_thumbnails", "matrix_coeffs",
            "full_range", "item_id", "aux_item_id",
        )
    ]


class TileParams(ctypes.Structure):
    """heifgpu_tile_params (parsed SPS/PPS/slice header of one tile)."""
    _fields_ = [(name, ctypes.c_int32) for name in (
            "nal_unit_type",
            "slice_type",
            "first_slice_segment_in_pic",
            "general_profile_idc",
            "general_level_idc",
            "pic_width",
            "pic_height",
            "chroma_format_idc",
            "bit_depth_luma",
            "bit_depth_chroma",
            "log2_max_poc_lsb",
            "log2_min_cb",
            "log2_ctb",
            "log2_min_tb",
            "log2_max_tb",
            "max_th_depth_inter",
            "max_th_depth_intra",
            "scaling_list_enabled",
            "amp",
            "sao",
            "pcm",
            "num_short_term_ref_pic_sets",
            "long_term_refs",
            "temporal_mvp",
            "strong_intra_smoothing",
            "video_full_range",
            "colour_primaries",
            "transfer_characteristics",
            "matrix_coeffs",
            "init_qp",
            "sign_data_hiding",
            "cabac_init_present",
            "constrained_intra_pred",
            "transform_skip",
            "cu_qp_delta_enabled",
            "diff_cu_qp_delta_depth",
            "cb_qp_offset",
            "cr_qp_offset",
            "slice_chroma_qp_offsets_present",
            "transquant_bypass",
            "tiles_enabled",
            "entropy_coding_sync",
            "loop_filter_across_slices",
            "deblocking_control_present",
            "deblocking_override_enabled",
            "deblocking_disabled",
            "beta_offset_div2",
            "tc_offset_div2",
            "log2_parallel_merge_level",
            "slice_sao_luma",
            "slice_sao_chroma",
            "slice_qp_y",
            "num_entry_point_offsets",
            "slice_data_raw_offset",
            "payload_bytes",
    )] + [("entry_point_offset", ctypes.c_uint32 * 64)]


class Planes(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int32 * 3)]


class BatchOpts(ctypes.Structure):
    """heifgpu_batch_opts: decode only grid tiles k with k % tile_stride == tile_offset;
    parse_mode (PARSE_*) and, in lanes mode, pictures per wave (0 = adaptive)."""
    _fields_ = [("tile_stride", ctypes.c_uint32), ("tile_offset", ctypes.c_uint32),
                ("parse_mode", ctypes.c_uint32), ("pics_per_wave", ctypes.c_uint32),
                ("pipeline_sets", ctypes.c_uint32)]


class IpcHandle(ctypes.Structure):
    """heifgpu_ipc_handle: a device allocation exported to another process."""
    _fields_ = [("handle", ctypes.c_uint8 * 64), ("offset", ctypes.c_uint64)]


class DisplayInfo(ctypes.Structure):
    """heifgpu_display_info: displayed size, the folded clap / irot / imir map
    (output pixel (ox, oy) shows decoded sample (m0*ox + m1*oy + t0, m2*ox + m3*oy + t1))
    and the alpha auxiliary image."""
    _fields_ = [("out_width", ctypes.c_uint32), ("out_height", ctypes.c_uint32),
                ("m", ctypes.c_int32 * 4), ("t", ctypes.c_int32 * 2),
                ("n_transforms", ctypes.c_uint32), ("alpha_item_id", ctypes.c_uint32),
                ("alpha_premultiplied", ctypes.c_uint32)]


class Surface(ctypes.Structure):
    """heifgpu_surface: interleaved output pixels on the device, bytes per row."""
    _fields_ = [("pixels", ctypes.c_void_p), ("pitch", ctypes.c_int32)]


class Scale(ctypes.Structure):
    """heifgpu_scale: rendered size and the window of the displayed picture it
    shows (width == height == 0: the whole picture)."""
    _fields_ = [("out_width", ctypes.c_uint32), ("out_height", ctypes.c_uint32),
                ("x", ctypes.c_uint32), ("y", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]


class Rect(ctypes.Structure):
    """heifgpu_rect: a rectangle of samples (width == height == 0: everything)."""
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32)]

    def as_tuple(self):
        return (self.x, self.y, self.width, self.height)


class TensorFormat(ctypes.Structure):
    """heifgpu_tensor_format: the integer format the picture is rendered in, the
    element type and layout it is written as, and out = R * a[c] + b[c]."""
    _fields_ = [("src", ctypes.c_uint32), ("elem", ctypes.c_uint32), ("layout", ctypes.c_uint32),
                ("a", ctypes.c_float * 4), ("b", ctypes.c_float * 4)]


class TensorSurface(ctypes.Structure):
    """heifgpu_tensor_surface: one image's elements on the device, strides in bytes."""
    _fields_ = [("data", ctypes.c_void_p), ("stride_c", ctypes.c_int64), ("stride_y", ctypes.c_int64)]


class ColorInfo(ctypes.Structure):
    """heifgpu_color_info: what defines an image's colour space (kind: COLOR_*), its
    nclx codes, the profile's size, what a transform of it would answer (status) and,
    when that is HEIFGPU_OK, the source colourants: X Y Z of R, of G, of B (D50)."""
    _fields_ = [("kind", ctypes.c_uint32), ("has_nclx", ctypes.c_uint32), ("primaries", ctypes.c_uint32),
                ("transfer", ctypes.c_uint32), ("icc_size", ctypes.c_uint32), ("status", ctypes.c_int32),
                ("colorants", ctypes.c_double * 9)]


class ColorTransform(ctypes.Structure):
    """heifgpu_color_transform: the tables and the Q14 matrix of one source at one depth."""
    _fields_ = [("bits", ctypes.c_uint32), ("identity", ctypes.c_uint32), ("dst", ctypes.c_uint32),
                ("tone", ctypes.c_uint32), ("m", ctypes.c_int32 * 9), ("m_rounded", ctypes.c_int32 * 9),
                ("in_lut", (ctypes.c_uint16 * 4096) * 3), ("out_lut", ctypes.c_uint16 * 4098)]


class HdrInfo(ctypes.Structure):
    """heifgpu_hdr_info: the transfer of an nclx-defined PQ / HLG item (else 0), which of
    clli / mdcv it carries (present: HDR_HAS_*), their values, and what a tone transform
    of the item answers (status)."""
    _fields_ = [("transfer", ctypes.c_uint32), ("present", ctypes.c_uint32), ("max_cll", ctypes.c_uint32),
                ("max_fall", ctypes.c_uint32), ("mastering_max", ctypes.c_uint32), ("mastering_min", ctypes.c_uint32),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class HdrTransform(ctypes.Structure):
    """heifgpu_hdr_transform: a colour transform (base; base.tone != 0) and the tables of
    its tone stage.  A render or heifgpu_color_apply takes the address of `base`."""
    _fields_ = [("base", ColorTransform), ("in_lut32", (ctypes.c_uint32 * 4096) * 3), ("w", ctypes.c_int32 * 3),
                ("transfer", ctypes.c_uint32), ("T", ctypes.c_uint32 * 578), ("Lsrc", ctypes.c_double)]

    # what the renders read of a transform, whichever kind it is
    bits = property(lambda self: self.base.bits)
    identity = property(lambda self: self.base.identity)
    dst = property(lambda self: self.base.dst)
    tone = property(lambda self: self.base.tone)


COLOR_NONE, COLOR_ICC, COLOR_NCLX = 0, 1, 2
COLOR_KINDS = {COLOR_NONE: "none", COLOR_ICC: "icc", COLOR_NCLX: "nclx"}
CS_SRGB, CS_DISPLAY_P3 = 0, 1
COLORSPACES = {"srgb": CS_SRGB, "display-p3": CS_DISPLAY_P3}
TONE_NONE, TONE_BT2390 = 0, 1
TONE_MAPS = {"bt2390": TONE_BT2390}
HDR_HAS_CLLI, HDR_HAS_MDCV = 1, 2
TONE_ENTRIES = 577

ELEM_F32, ELEM_F16, ELEM_BF16 = 0, 1, 2
LAYOUT_CHW, LAYOUT_HWC = 0, 1
LAYOUTS = {"chw": LAYOUT_CHW, "hwc": LAYOUT_HWC}

FILTER_AREA, FILTER_BILINEAR, FILTER_BICUBIC = 0, 1, 2
FILTERS = {"area": FILTER_AREA, "bilinear": FILTER_BILINEAR, "bicubic": FILTER_BICUBIC}

FIT_STRETCH, FIT_CONTAIN, FIT_COVER = 0, 1, 2
FIT_MODES = {"stretch": FIT_STRETCH, "contain": FIT_CONTAIN, "cover": FIT_COVER}

PIX_RGB8, PIX_RGBA8, PIX_RGB16, PIX_RGBA16 = 0, 1, 2, 3
PIX_FORMATS = {"rgb8": PIX_RGB8, "rgba8": PIX_RGBA8, "rgb16": PIX_RGB16, "rgba16": PIX_RGBA16}

class ChromaInfo(ctypes.Structure):  # heifgpu_chroma_info
    _fields_ = [("loc", ctypes.c_uint32), ("signalled", ctypes.c_uint32), ("loc_override", ctypes.c_int32),
                ("mode", ctypes.c_uint32), ("sub_width_c", ctypes.c_uint32), ("sub_height_c", ctypes.c_uint32)]


CHROMA_REPLICATE, CHROMA_BILINEAR = 0, 1
CHROMA_MODES = {"replicate": CHROMA_REPLICATE, "bilinear": CHROMA_BILINEAR}


class GainInfo(ctypes.Structure):
    """heifgpu_gain_info: the kind of an image's gain map (GAIN_*), the gain-map image item,
    what a transform answers (status) and the fields of an ISO 21496-1 'tmap' payload."""
    _fields_ = [("kind", ctypes.c_uint32), ("gain_item_id", ctypes.c_uint32), ("status", ctypes.c_int32),
                ("version", ctypes.c_uint32), ("minimum_version", ctypes.c_uint32), ("writer_version", ctypes.c_uint32),
                ("multichannel", ctypes.c_uint32), ("use_base_colour_space", ctypes.c_uint32),
                ("base_headroom", ctypes.c_double), ("alternate_headroom", ctypes.c_double),
                ("gain_min", ctypes.c_double), ("gain_max", ctypes.c_double), ("gamma", ctypes.c_double),
                ("base_offset", ctypes.c_double), ("alternate_offset", ctypes.c_double)]


GAIN_T_ENTRIES, GAIN_E_ENTRIES = 4097, 641


class GainTransform(ctypes.Structure):
    """heifgpu_gain_transform: the tables, the Q14 matrix and the offsets of one base image
    with its gain map, for one destination and one encoding."""
    _fields_ = [("bits", ctypes.c_uint32), ("gain_bits", ctypes.c_uint32), ("dst", ctypes.c_uint32),
                ("encoding", ctypes.c_uint32), ("pq_bits", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("m", ctypes.c_int32 * 9), ("k_b", ctypes.c_int32), ("k_a", ctypes.c_int32),
                ("weight", ctypes.c_double), ("headroom", ctypes.c_double), ("sdr_white", ctypes.c_double),
                ("in_lut", (ctypes.c_uint16 * 4096) * 3), ("T", ctypes.c_uint32 * (GAIN_T_ENTRIES + 1)),
                ("E", ctypes.c_uint32 * (GAIN_E_ENTRIES + 1))]


GAIN_NONE, GAIN_APPLE, GAIN_ISO = 0, 1, 2
GAIN_KINDS = {GAIN_NONE: "none", GAIN_APPLE: "apple", GAIN_ISO: "iso"}
CS_BT2020 = 2  # a destination of the gain-map HDR render only
HDR_COLORSPACES = {"srgb": 0, "display-p3": 1, "bt2020": CS_BT2020}
GAIN_LINEAR, GAIN_PQ = 0, 1
PIX_HDR_RGB16F, PIX_HDR_RGBA16F, PIX_HDR_RGB16PQ, PIX_HDR_RGBA16PQ = 4, 5, 6, 7
HDR_FORMATS = {"rgb16f": PIX_HDR_RGB16F, "rgba16f": PIX_HDR_RGBA16F, "rgb16pq": PIX_HDR_RGB16PQ,
               "rgba16pq": PIX_HDR_RGBA16PQ}

class JpegOpts(ctypes.Structure):
    """heifgpu_jpeg_opts: quality 1..100, JPEG_444 / JPEG_420, MCUs per restart interval (0: a row)."""
    _fields_ = [("quality", ctypes.c_uint32), ("subsampling", ctypes.c_uint32), ("restart_mcus", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


JPEG_444, JPEG_420 = 0, 1
JPEG_SUBSAMPLINGS = {"4:4:4": JPEG_444, "4:2:0": JPEG_420}
JPEG_TOO_SMALL = 1 << 63  # a bit of heifgpu_jpeg_encode_batch's sizes


class PngOpts(ctypes.Structure):
    """heifgpu_png_opts: a render format, the significant bits of a 16-bit one, filter 0..5."""
    _fields_ = [("format", ctypes.c_uint32), ("bits", ctypes.c_uint32), ("filter", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class PngColour(ctypes.Structure):
    """heifgpu_png_colour: which of sRGB / cICP / iCCP the header carries."""
    _fields_ = [("kind", ctypes.c_uint32), ("cicp", ctypes.c_uint8 * 4), ("icc", ctypes.POINTER(ctypes.c_uint8)),
                ("icc_len", ctypes.c_size_t)]


PNG_COLOUR_NONE, PNG_COLOUR_SRGB, PNG_COLOUR_CICP, PNG_COLOUR_ICC = 0, 1, 2, 3
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
PNG_TOO_SMALL = 1 << 63  # a bit of heifgpu_png_encode_batch's sizes
PNG_BLOCK = 32768        # filtered bytes per deflate block (one IDAT chunk each)

PARSE_AUTO, PARSE_LANES, PARSE_SOLO, PARSE_SPREAD = 0, 1, 2, 3
PARSE_ROWS = 4  # ABI 5 only; removed in ABI 6 (prepare answers HEIFGPU_E_UNSUPPORTED)
PARSE_MODES = {"auto": PARSE_AUTO, "lanes": PARSE_LANES, "solo": PARSE_SOLO, "spread": PARSE_SPREAD}
ABI_VERSION = 6  # HEIFGPU_ABI_VERSION of include/heifgpu.h these declarations follow


# every symbol include/heifgpu.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "heifgpu_image_parse", "heifgpu_image_get_info", "heifgpu_image_free", "heifgpu_create",
    "heifgpu_destroy", "heifgpu_last_error", "heifgpu_batch_prepare", "heifgpu_batch_decode",
    "heifgpu_batch_status", "heifgpu_batch_free", "heifgpu_set_timing", "heifgpu_stage_times",
    "heifgpu_decode_batch", "heifgpu_remove_emulation_prevention", "heifgpu_read_ue",
    "heifgpu_read_se", "heifgpu_bins_truncated_rice", "heifgpu_bins_chroma_pred_mode",
    "heifgpu_bins_coeff_abs_level_remaining", "heifgpu_bins_exp_golomb", "heifgpu_image_tile_params", "heifgpu_debug_counters",
    "heifgpu_image_parse_item", "heifgpu_ycbcr_to_rgb", "heifgpu_batch_prepare_ex", "heifgpu_gather_tiles",
    "heifgpu_image_parse_many", "heifgpu_batch_parse_geometry", "heifgpu_ipc_export", "heifgpu_ipc_open",
    "heifgpu_ipc_close", "heifgpu_batch_status_previous", "heifgpu_abi_version", "heifgpu_batch_lanes_variant",
    "heifgpu_image_get_display", "heifgpu_render_batch", "heifgpu_scale_fit", "heifgpu_render_batch_scaled",
    "heifgpu_render_batch_tensor", "heifgpu_window_source_rect", "heifgpu_image_tiles_for_rect",
    "heifgpu_batch_prepare_rects", "heifgpu_batch_count_pictures", "heifgpu_batch_picture_count",
    "heifgpu_image_get_color", "heifgpu_image_get_icc", "heifgpu_color_transform_make", "heifgpu_color_apply",
    "heifgpu_render_batch_color", "heifgpu_render_batch_scaled_color", "heifgpu_render_batch_tensor_color",
    "heifgpu_render_batch_resampled", "heifgpu_render_batch_tensor_resampled", "heifgpu_resample_coeffs",
    "heifgpu_resample_apply", "heifgpu_window_source_rect_resampled",
    "heifgpu_image_get_hdr", "heifgpu_color_transform_make_hdr",
    "heifgpu_image_get_chroma", "heifgpu_image_set_chroma_upsampling", "heifgpu_chroma_upsample",
    "heifgpu_image_get_gain", "heifgpu_gain_transform_make", "heifgpu_gain_apply", "heifgpu_gain_sample",
    "heifgpu_render_batch_gain", "heifgpu_render_batch_gain_scaled", "heifgpu_gain_average",
    "heifgpu_jpeg_quant_tables", "heifgpu_jpeg_header", "heifgpu_jpeg_encode_host", "heifgpu_jpeg_encode_batch",
    "heifgpu_render_batch_scaled_linear", "heifgpu_render_batch_tensor_linear", "heifgpu_linear_average_apply",
    "heifgpu_png_header", "heifgpu_png_encode_host", "heifgpu_png_encode_batch",
)


class HeifGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"heifgpu error {code}: {msg}")
        self.code = code


class UnsupportedError(HeifGpuError):
    pass


def _bind_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64;
    if libheifgpu.so were loaded first it would pull /opt/rocm's copy and the
    two runtimes cannot share the device (whichever initialises second sees
    no GPU).  Importing torch first makes the dynamic linker bind
    libheifgpu.so's libamdhip64.so.7 dependency to torch's already-loaded
    copy.  Without torch (e.g. a C/Rust host) nothing changes."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def _load() -> ctypes.CDLL:
    _bind_hip_runtime()
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback on the product path)"
        )
    lib = ctypes.CDLL(str(LIB_PATH), mode=os.RTLD_LOCAL)
    P, VP, SZ, I32, U32 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    u8p = P(ctypes.c_uint8)
    sig = {
        "heifgpu_image_parse": (I32, [u8p, SZ, P(VP)]),
        "heifgpu_image_get_info": (I32, [VP, P(ImageInfo)]),
        "heifgpu_image_free": (None, [VP]),
        "heifgpu_create": (I32, [I32, P(VP)]),
        "heifgpu_destroy": (None, [VP]),
        "heifgpu_last_error": (ctypes.c_char_p, []),
        "heifgpu_batch_prepare": (I32, [VP, P(VP), SZ, P(VP)]),
        "heifgpu_batch_decode": (I32, [VP, VP, P(Planes), VP]),
        "heifgpu_batch_status": (I32, [VP, VP, P(U32), VP]),
        "heifgpu_batch_status_previous": (I32, [VP, VP, P(U32), SZ, P(SZ), VP]),
        "heifgpu_abi_version": (I32, []),
        "heifgpu_batch_free": (None, [VP]),
        "heifgpu_set_timing": (I32, [VP, I32]),
        "heifgpu_stage_times": (I32, [VP, P(ctypes.c_float)]),
        "heifgpu_decode_batch": (I32, [VP, P(VP), SZ, P(Planes), VP, P(U32)]),
        "heifgpu_remove_emulation_prevention": (SZ, [u8p, SZ, u8p]),
        "heifgpu_read_ue": (I32, [u8p, SZ, P(U32)]),
        "heifgpu_read_se": (I32, [u8p, SZ, P(ctypes.c_int32)]),
        "heifgpu_bins_truncated_rice": (I32, [u8p, I32, I32, I32, P(I32)]),
        "heifgpu_bins_chroma_pred_mode": (I32, [u8p, I32, P(I32)]),
        "heifgpu_bins_coeff_abs_level_remaining": (I32, [u8p, I32, I32, P(I32)]),
        "heifgpu_bins_exp_golomb": (I32, [u8p, I32, I32, P(I32)]),
        "heifgpu_image_tile_params": (I32, [VP, U32, P(TileParams)]),
        "heifgpu_debug_counters": (I32, [P(ctypes.c_uint64), I32]),
        "heifgpu_image_parse_item": (I32, [u8p, SZ, U32, P(VP)]),
        "heifgpu_ycbcr_to_rgb": (I32, [VP, P(ImageInfo), P(Planes), VP, I32, VP]),
        "heifgpu_batch_prepare_ex": (I32, [VP, P(VP), SZ, P(BatchOpts), P(VP)]),
        "heifgpu_gather_tiles": (I32, [P(ImageInfo), P(Planes), P(Planes), U32, U32, VP]),
        "heifgpu_image_parse_many": (I32, [P(P(ctypes.c_uint8)), P(SZ), SZ, I32, P(VP), P(I32)]),
        "heifgpu_batch_parse_geometry": (I32, [VP, P(U32), P(U32), P(U32), P(U32)]),
        "heifgpu_ipc_export": (I32, [VP, P(IpcHandle)]),
        "heifgpu_ipc_open": (I32, [I32, P(IpcHandle), P(VP)]),
        "heifgpu_ipc_close": (I32, [VP]),
        "heifgpu_batch_lanes_variant": (I32, [VP, P(U32)]),
        "heifgpu_image_get_display": (I32, [VP, P(DisplayInfo)]),
        "heifgpu_render_batch": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(Surface), VP]),
        "heifgpu_scale_fit": (I32, [P(DisplayInfo), U32, U32, U32, P(Scale)]),
        "heifgpu_render_batch_scaled": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(Scale), P(Surface),
                                              VP]),
        "heifgpu_render_batch_tensor": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(TensorFormat), P(Scale),
                                              P(U32), P(TensorSurface), VP]),
        "heifgpu_window_source_rect": (I32, [VP, P(Rect), P(Rect)]),
        "heifgpu_image_tiles_for_rect": (I32, [VP, P(Rect), P(U32), P(U32), P(U32), P(U32)]),
        "heifgpu_batch_prepare_rects": (I32, [VP, P(VP), SZ, P(BatchOpts), P(Rect), P(VP)]),
        "heifgpu_batch_count_pictures": (I32, [P(VP), SZ, P(BatchOpts), P(Rect), P(U32)]),
        "heifgpu_batch_picture_count": (I32, [VP, P(U32)]),
        "heifgpu_image_get_color": (I32, [VP, P(ColorInfo)]),
        "heifgpu_image_get_icc": (I32, [VP, u8p, SZ, P(SZ)]),
        "heifgpu_color_transform_make": (I32, [VP, U32, U32, P(ColorTransform)]),
        "heifgpu_color_apply": (I32, [P(ColorTransform), P(ctypes.c_uint16), SZ, P(ctypes.c_uint16)]),
        "heifgpu_render_batch_color": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(VP), P(Surface), VP]),
        "heifgpu_render_batch_scaled_color": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(Scale), P(VP),
                                                    P(Surface), VP]),
        "heifgpu_render_batch_tensor_color": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(TensorFormat), P(Scale),
                                                    P(U32), P(VP), P(TensorSurface), VP]),
        "heifgpu_render_batch_resampled": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(Scale), U32, P(VP),
                                                 P(Surface), VP]),
        "heifgpu_render_batch_tensor_resampled": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(TensorFormat),
                                                        P(Scale), U32, P(U32), P(VP), P(TensorSurface), VP]),
        "heifgpu_resample_coeffs": (I32, [U32, U32, U32, U32, U32, U32, P(ctypes.c_int32), P(ctypes.c_int32), SZ, P(U32)]),
        "heifgpu_resample_apply": (I32, [VP, U32, U32, U32, U32, P(Rect), U32, U32, U32, VP]),
        "heifgpu_window_source_rect_resampled": (I32, [VP, P(Scale), U32, P(Rect)]),
        "heifgpu_image_get_hdr": (I32, [VP, P(HdrInfo)]),
        "heifgpu_color_transform_make_hdr": (I32, [VP, U32, U32, U32, ctypes.c_double, P(HdrTransform)]),
        "heifgpu_image_get_chroma": (I32, [VP, P(ChromaInfo)]),
        "heifgpu_image_set_chroma_upsampling": (I32, [VP, U32, ctypes.c_int32]),
        "heifgpu_chroma_upsample": (I32, [VP, U32, U32, ctypes.c_int32, U32, U32, U32, U32, U32, U32, U32, VP,
                                          ctypes.c_int32]),
        "heifgpu_image_get_gain": (I32, [VP, P(GainInfo)]),
        "heifgpu_gain_transform_make": (I32, [VP, VP, U32, U32, U32, U32, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_double, P(GainTransform)]),
        "heifgpu_gain_apply": (I32, [P(GainTransform), P(ctypes.c_uint16), P(U32), SZ, P(ctypes.c_uint16)]),
        "heifgpu_gain_sample": (I32, [VP, U32, U32, ctypes.c_int32, U32, U32, U32, P(U32)]),
        "heifgpu_render_batch_gain": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(VP), P(Planes), U32, P(VP),
                                            P(Surface), VP]),
        "heifgpu_render_batch_gain_scaled": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(VP), P(Planes), U32,
                                                   P(Scale), P(VP), P(Surface), VP]),
        "heifgpu_gain_average": (I32, [P(U32), U32, U32, P(Scale), P(U32)]),
        "heifgpu_jpeg_quant_tables": (I32, [U32, u8p, u8p]),
        "heifgpu_jpeg_header": (I32, [U32, U32, P(JpegOpts), u8p, SZ, u8p, SZ, P(SZ)]),
        "heifgpu_jpeg_encode_host": (I32, [VP, ctypes.c_int32, U32, U32, P(JpegOpts), u8p, SZ, u8p, SZ, P(SZ)]),
        "heifgpu_jpeg_encode_batch": (I32, [VP, SZ, P(Surface), P(U32), P(U32), P(JpegOpts), P(Surface),
                                            P(ctypes.c_uint64), VP]),
        "heifgpu_render_batch_scaled_linear": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), U32, P(Scale), P(VP),
                                                     P(Surface), VP]),
        "heifgpu_render_batch_tensor_linear": (I32, [VP, P(VP), SZ, P(Planes), P(VP), P(Planes), P(TensorFormat), P(Scale),
                                                     P(U32), P(VP), P(TensorSurface), VP]),
        "heifgpu_linear_average_apply": (I32, [P(ColorTransform), P(ctypes.c_uint16), U32, U32, U32, P(Rect), U32, U32,
                                               P(ctypes.c_uint16)]),
        "heifgpu_png_header": (I32, [U32, U32, P(PngOpts), P(PngColour), u8p, SZ, P(SZ)]),
        "heifgpu_png_encode_host": (I32, [VP, ctypes.c_int32, U32, U32, P(PngOpts), P(PngColour), u8p, SZ, P(SZ)]),
        "heifgpu_png_encode_batch": (I32, [VP, SZ, P(Surface), P(U32), P(U32), P(PngOpts), P(Surface),
                                           P(ctypes.c_uint64), VP]),
    }
    # added within ABI 6: an earlier build of it (HEIFGPU_LIBRARY, a same-box A/B) has one lanes body
    # (and no window decode: DecodeContext.prepare without windows then goes through prepare_ex)
    optional = {"heifgpu_batch_lanes_variant", "heifgpu_window_source_rect", "heifgpu_image_tiles_for_rect",
                "heifgpu_batch_prepare_rects", "heifgpu_batch_count_pictures", "heifgpu_batch_picture_count",
                # the colour-managed render (colorspace= then needs a build that has it)
                "heifgpu_image_get_color", "heifgpu_image_get_icc", "heifgpu_color_transform_make", "heifgpu_color_apply",
                "heifgpu_render_batch_color", "heifgpu_render_batch_scaled_color", "heifgpu_render_batch_tensor_color",
                # the filtered renders (filter= other than "area" then needs a build that has them)
                "heifgpu_render_batch_resampled", "heifgpu_render_batch_tensor_resampled", "heifgpu_resample_coeffs",
                "heifgpu_resample_apply", "heifgpu_window_source_rect_resampled",
                # the HDR render (tone_map= then needs a build that has it)
                "heifgpu_image_get_hdr", "heifgpu_color_transform_make_hdr",
                # bilinear chroma upsampling (chroma= other than "replicate" then needs a build that has it)
                "heifgpu_image_get_chroma", "heifgpu_image_set_chroma_upsampling", "heifgpu_chroma_upsample",
                # the gain-map HDR render (render_hdr / decode_hdr then need a build that has it)
                "heifgpu_image_get_gain", "heifgpu_gain_transform_make", "heifgpu_gain_apply", "heifgpu_gain_sample",
                "heifgpu_render_batch_gain",
                # its scaled form (render_hdr_scaled / decode_hdr(size=) then need a build that has it)
                "heifgpu_render_batch_gain_scaled", "heifgpu_gain_average",
                # the JPEG output (encode_jpeg / render_jpeg / decode_jpeg then need a build that has it)
                "heifgpu_jpeg_quant_tables", "heifgpu_jpeg_header", "heifgpu_jpeg_encode_host",
                "heifgpu_jpeg_encode_batch",
                # the linear-light scaled renders (linear=True then needs a build that has them)
                "heifgpu_render_batch_scaled_linear", "heifgpu_render_batch_tensor_linear",
                "heifgpu_linear_average_apply",
                # the PNG output (encode_png / render_png / decode_png then need a build that has it)
                "heifgpu_png_header", "heifgpu_png_encode_host", "heifgpu_png_encode_batch"}
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # the structs above follow ABI_VERSION: a library of another version must not be called
    got = lib.heifgpu_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: library ABI {got}, these bindings expect {ABI_VERSION} (rebuild it)")
    return lib


lib = _load()


def last_error() -> str:
    return lib.heifgpu_last_error().decode(errors="replace")


def check(rc: int) -> None:
    if rc == HEIFGPU_OK:
        return
    if rc == HEIFGPU_E_UNSUPPORTED:
        raise UnsupportedError(rc, last_error())
    raise HeifGpuError(rc, last_error())


def u8buf(data: bytes):
    return (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
