"""ctypes bindings to the in-tree native libraries.

libh264mi.so  -- product: host parser + HIP reconstruction engine + C-ABI
                 (include/h264mi.h).  No CPU reconstruction exists in it.
libh264gen.so -- seeded synthetic Baseline stream generator (test/bench input).

The libraries are built by ``__graft_entry__.build()`` (or ``make -C
broadway_amd/csrc``) into ``broadway_amd/lib``.  Loading fails loudly when a
library is missing: there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import os

# H264MI_LIB_DIR: load another build of the same libraries (A/B timing of
# kernel variants in one process tree; tools/ab.sh)
LIB_DIR = os.environ.get("H264MI_LIB_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")


class NativeLibraryMissing(RuntimeError):
    pass


def _load(name: str) -> C.CDLL:
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise NativeLibraryMissing(
            f"{path} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_mi = None
_gen = None


# ---------------------------------------------------------------- structs ---
class H264SwDecInput(C.Structure):
    _fields_ = [("pStream", C.POINTER(C.c_uint8)), ("dataLen", C.c_uint32),
                ("picId", C.c_uint32), ("intraConcealmentMethod", C.c_uint32)]


class H264SwDecOutput(C.Structure):
    _fields_ = [("pStrmCurrPos", C.POINTER(C.c_uint8))]


class H264SwDecPicture(C.Structure):
    _fields_ = [("pOutputPicture", C.POINTER(C.c_uint32)), ("picId", C.c_uint32),
                ("isIdrPicture", C.c_uint32), ("nbrOfErrMBs", C.c_uint32)]


class CropParams(C.Structure):
    _fields_ = [("cropLeftOffset", C.c_uint32), ("cropOutWidth", C.c_uint32),
                ("cropTopOffset", C.c_uint32), ("cropOutHeight", C.c_uint32)]


class H264SwDecInfo(C.Structure):
    _fields_ = [("profile", C.c_uint32), ("picWidth", C.c_uint32), ("picHeight", C.c_uint32),
                ("videoRange", C.c_uint32), ("matrixCoefficients", C.c_uint32),
                ("parWidth", C.c_uint32), ("parHeight", C.c_uint32),
                ("croppingFlag", C.c_uint32), ("cropParams", CropParams)]


class H264SwDecApiVersion(C.Structure):
    _fields_ = [("major", C.c_uint32), ("minor", C.c_uint32)]


class GenParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "w_mbs", "h_mbs", "crop_right", "crop_bottom", "nframes", "gop", "slices",
        "pm_skip", "pm_16x16", "pm_16x8", "pm_8x16", "pm_8x8", "pm_intra", "p8x8_ref0_pct",
        "im_i4", "im_i16", "im_pcm", "i4_rem_pct", "qp_min", "qp_max", "qp_delta",
        "dbf_idc1_pct", "dbf_idc2_pct", "dbf_off", "num_ref_frames", "cip", "chroma_qp_offset",
        "poc_type", "coef_pct", "level_tail_pct", "mv_jitter", "offpic_pct",
        "log2_max_frame_num", "poc_swap",
        "err_range_pct", "drop_slice_pct", "trunc_slice_pct", "drop_pic_pct", "gaps_allowed",
        "nonref_pct", "ref_mod_pct", "mmco_pct", "lt_idr_pct", "crop_left", "crop_top",
        "vui_matrix", "vui_full_range")] + [("seed", C.c_uint64)]


class TensorDesc(C.Structure):
    """h264mi_tensor_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "cw", "ch", "mode", "dtype")] + \
               [("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class TensorResizeDesc(C.Structure):
    """h264mi_tensor_resize_desc (include/h264mi.h)."""
    _fields_ = [("t", TensorDesc), ("ow", C.c_int), ("oh", C.c_int), ("filter", C.c_int)]


class Roi(C.Structure):
    """h264mi_roi (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("pic", "x", "y", "cw", "ch")]


class TensorFitDesc(C.Structure):
    """h264mi_tensor_fit_desc (include/h264mi.h)."""
    _fields_ = [("r", TensorResizeDesc), ("fit", C.c_int), ("pad", C.c_ubyte * 4)]


class TensorLayoutDesc(C.Structure):
    """h264mi_tensor_layout_desc (include/h264mi.h)."""
    _fields_ = [("f", TensorFitDesc), ("layout", C.c_int)]


class TensorDest(C.Structure):
    """h264mi_tensor_dest (include/h264mi.h): a pixel export's strides, in bytes."""
    _fields_ = [("row", C.c_int64), ("plane", C.c_int64), ("frame", C.c_int64), ("clip", C.c_int32),
                ("reserved", C.c_int32)]


class Warp(C.Structure):
    """h264mi_warp (include/h264mi.h)."""
    _fields_ = [("pic", C.c_int), ("m", C.c_int * 6)]


class TensorWarpDesc(C.Structure):
    """h264mi_tensor_warp_desc (include/h264mi.h)."""
    _fields_ = [("t", TensorDesc)] + [(n, C.c_int) for n in ("ow", "oh", "filter", "border")] + \
               [("pad", C.c_ubyte * 4), ("layout", C.c_int)]


class StatsDesc(C.Structure):
    """h264mi_stats_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "cw", "ch", "planes", "colour", "flags", "reserved")]


class MbInfoDesc(C.Structure):
    """h264mi_mbinfo_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("bx", "by", "bw", "bh", "nch", "dtype")] + \
               [("ch", C.c_int * 16), ("scale", C.c_float * 16), ("bias", C.c_float * 16)]


class ResidualDesc(C.Structure):
    """h264mi_residual_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "cw", "ch", "planes", "dtype")] + \
               [("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class AccMvDesc(C.Structure):
    """h264mi_accmv_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "cw", "ch", "nch", "dtype")] + \
               [("id", C.c_int * 8), ("scale", C.c_float * 8), ("bias", C.c_float * 8)]


class AccResDesc(C.Structure):
    """h264mi_accres_desc (include/h264mi.h)."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "cw", "ch", "planes", "dtype", "colour", "unanchored")] + \
               [("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class AccMvResizeDesc(C.Structure):
    """h264mi_accmv_resize_desc (include/h264mi.h)."""
    _fields_ = [("f", AccMvDesc), ("ow", C.c_int), ("oh", C.c_int), ("filter", C.c_int)]


class AccResResizeDesc(C.Structure):
    """h264mi_accres_resize_desc (include/h264mi.h)."""
    _fields_ = [("f", AccResDesc), ("ow", C.c_int), ("oh", C.c_int), ("filter", C.c_int)]


# channel ids of AccMvDesc.id, by name
ACCMV_CHANNELS = {"adx": 0, "ady": 1, "jx": 2, "jy": 3, "anchored": 4}
ACCMV_MAX_CH = 8

# AccResDesc.planes and .unanchored, by name
ACCRES_PLANES = {"y": 0, "uv": 1, "yuv": 2, "rgb": 3}
ACCRES_UNANCHORED = {"key": 0, "zero": 1}
ACCRES_MAX_KEYS = 8

# ResidualDesc.planes, by name
RESID_PLANES = {"y": 0, "uv": 1, "yuv": 2}

# channel ids of MbInfoDesc.ch, by name, and the int16 element type
MBINFO_CHANNELS = {"mvx": 0, "mvy": 1, "ref_idx": 2, "ref_slot": 3, "mb_type": 4, "qp": 5, "intra_mode": 6,
                   "coded": 7, "slice": 8}
MBINFO_MAX_CH = 16
TENSOR_I16 = 4

TENSOR_RGB, TENSOR_GRAY = 0, 1
# the colour set of an RGB tensor, bits 8..11 of TensorDesc.mode, by name; with
# "stream", bits 12..13 say what to take where the stream names no matrix
TENSOR_COLOURS = {"reference": 0, "bt601-full": 1, "bt709": 2, "bt709-full": 3, "stream": 15}
TENSOR_COLOUR_NAMES = ("reference", "bt601-full", "bt709", "bt709-full")
TENSOR_COLOUR_STREAM = 15
TENSOR_UNSPECIFIED = {"bt601": 0, "bt709": 1, "size": 2}
TENSOR_COLOUR_SHIFT, TENSOR_UNSPEC_SHIFT = 8, 12
RESIZE_TRIANGLE = 0
RESIZE_BICUBIC = 2            # (1 is reserved)
# TensorResizeDesc.filter by name, and the source samples per output and axis each takes at most
RESIZE_FILTERS = {"triangle": RESIZE_TRIANGLE, "bicubic": RESIZE_BICUBIC}
RESIZE_MAX_RATIO = {RESIZE_TRIANGLE: 32, RESIZE_BICUBIC: 16}
RESIZE_MAX_DIM = 16384
ROIS_MAX_PER_LAUNCH = 32
TENSOR_FIT = {"stretch": 0, "letterbox": 1, "topleft": 2}
TENSOR_U8, TENSOR_F16, TENSOR_BF16, TENSOR_F32 = 0, 1, 2, 3
# TensorLayoutDesc.layout by the name of the torch memory format it gives
TENSOR_LAYOUTS = {"nchw": 0, "nhwc": 1}
# TensorWarpDesc.filter and .border
WARP_BILINEAR = 0
WARP_BORDERS = {"constant": 0, "replicate": 1}
WARPS_MAX_PER_LAUNCH = 32
# StatsDesc.planes by name, its flag, and the int64 words of a plane record by name
STATS_PLANES = {"y": 0, "yuv": 1, "rgb": 2}
STATS_HIST = 1
STATS_WORDS, STATS_BINS = 8, 256
STATS_FIELDS = ("count", "sum", "sumsq", "min", "max", "sad", "ssd")

HEADERS_CB = C.CFUNCTYPE(None, C.c_void_p)
PICTURE_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32)

H264SWDEC_OK = 0
H264SWDEC_STRM_PROCESSED = 1
H264SWDEC_PIC_RDY = 2
H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY = 3
H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY = 4
H264SWDEC_PARAM_ERR = -1
H264SWDEC_STRM_ERR = -2
H264SWDEC_NOT_INITIALIZED = -3
H264SWDEC_MEMFAIL = -4
H264SWDEC_INITFAIL = -5
H264SWDEC_HDRS_NOT_RDY = -6


def mi() -> C.CDLL:
    """libh264mi.so with prototypes set.

    PyTorch-ROCm ships its own libamdhip64.so (same SONAME libamdhip64.so.7 as
    /opt/rocm's).  If torch is importable it is imported first so that
    libh264mi.so binds to that already-loaded runtime and the process holds a
    single HIP runtime (torch.cuda.synchronize() then sees our stream work)."""
    global _mi
    if _mi is not None:
        return _mi
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = _load("libh264mi.so")
    vp, i32, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    L.H264SwDecInit.argtypes = [C.POINTER(vp), u32]
    L.H264SwDecInit.restype = i32
    L.H264SwDecDecode.argtypes = [vp, C.POINTER(H264SwDecInput), C.POINTER(H264SwDecOutput)]
    L.H264SwDecDecode.restype = i32
    L.H264SwDecNextPicture.argtypes = [vp, C.POINTER(H264SwDecPicture), u32]
    L.H264SwDecNextPicture.restype = i32
    L.H264SwDecGetInfo.argtypes = [vp, C.POINTER(H264SwDecInfo)]
    L.H264SwDecGetInfo.restype = i32
    L.H264SwDecRelease.argtypes = [vp]
    L.H264SwDecRelease.restype = None
    L.H264SwDecGetAPIVersion.argtypes = []
    L.H264SwDecGetAPIVersion.restype = H264SwDecApiVersion
    L.broadwaySetCallbacks.argtypes = [HEADERS_CB, PICTURE_CB, vp]
    L.broadwaySetCallbacks.restype = None
    L.broadwayInit.restype = u32
    L.broadwayCreateStream.argtypes = [u32]
    L.broadwayCreateStream.restype = C.POINTER(C.c_uint8)
    L.broadwayPlayStream.argtypes = [u32]
    L.broadwayPlayStream.restype = None
    L.broadwayExit.restype = None
    L.broadwayGetMajorVersion.restype = u32
    L.broadwayGetMinorVersion.restype = u32
    L.h264mi_engine_create.argtypes = [i32, i32, i32, i32, i32]
    L.h264mi_engine_create.restype = vp
    L.h264mi_engine_destroy.argtypes = [vp]
    L.h264mi_engine_destroy.restype = None
    L.h264mi_engine_decode.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp),
                                       C.POINTER(vp), C.POINTER(u32)]
    L.h264mi_engine_decode.restype = i32
    L.h264mi_engine_decode_device.argtypes = [vp, i32, vp, vp, vp]
    L.h264mi_engine_decode_device.restype = i32
    L.h264mi_engine_hint_intra.argtypes = [vp, i32]
    L.h264mi_engine_hint_intra.restype = i32
    if hasattr(L, "h264mi_engine_hint_deps"):
        L.h264mi_engine_hint_deps.argtypes = [vp, i32]
        L.h264mi_engine_hint_deps.restype = i32
        L.h264mi_engine_last_deps.argtypes = [vp]
        L.h264mi_engine_last_deps.restype = i32
    if hasattr(L, "h264mi_engine_last_mc_waves"):
        L.h264mi_engine_last_mc_waves.argtypes = [vp]
        L.h264mi_engine_last_mc_waves.restype = i32
    L.h264mi_engine_decode_device_next.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.h264mi_engine_decode_device_next.restype = i32
    L.h264mi_engine_decode_device_steps.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.h264mi_engine_decode_device_steps.restype = i32
    if hasattr(L, "h264mi_engine_decode_device_steps_next"):
        L.h264mi_engine_decode_device_steps_next.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
        L.h264mi_engine_decode_device_steps_next.restype = i32
    L.h264mi_engine_set_steps.argtypes = [vp, i32]
    L.h264mi_engine_set_steps.restype = i32
    L.h264mi_set_share.argtypes = [i32]
    L.h264mi_set_share.restype = i32
    L.h264mi_share_stats.argtypes = [i32, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.h264mi_share_stats.restype = i32
    L.h264mi_engine_pool_stats.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.h264mi_engine_pool_stats.restype = None
    L.h264mi_engine_read.argtypes = [vp, i32, i32, vp]
    L.h264mi_engine_read.restype = i32
    L.h264mi_engine_read_rgba.argtypes = [vp, i32, i32, vp]
    L.h264mi_engine_read_rgba.restype = i32
    L.h264mi_yuv2rgba_device.argtypes = [vp, vp, i32, i32, i32, C.c_size_t, C.c_size_t, vp]
    L.h264mi_yuv2rgba_device.restype = i32
    if hasattr(L, "h264mi_yuv2rgba_device_pitch"):      # (absent from A/B builds of older trees)
        L.h264mi_yuv2rgba_device_pitch.argtypes = [vp, vp, i32, i32, i32, i32, C.c_size_t, C.c_size_t, vp]
        L.h264mi_yuv2rgba_device_pitch.restype = i32
    L.H264SwDecNextPictureRGBA.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, vp]
    L.H264SwDecNextPictureRGBA.restype = i32
    if hasattr(L, "h264mi_crop_device_pitch"):          # (optional: a library without them still loads)
        L.H264SwDecNextPictureCropped.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, vp, u32]
        L.H264SwDecNextPictureCropped.restype = i32
        L.h264mi_crop_device_pitch.argtypes = [vp, vp] + [i32] * 9 + [sz, sz, vp]
        L.h264mi_crop_device_pitch.restype = i32
        L.h264mi_engine_read_crop.argtypes = [vp] + [i32] * 7 + [vp]
        L.h264mi_engine_read_crop.restype = i32
    if hasattr(L, "h264mi_tensor_device_pitch"):        # (optional, as above)
        td = C.POINTER(TensorDesc)
        L.h264mi_tensor_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, td, vp, sz, vp]
        L.h264mi_tensor_device_pitch.restype = i32
        L.h264mi_engine_export_tensor.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), td, vp, sz, vp]
        L.h264mi_engine_export_tensor.restype = i32
        L.H264SwDecNextPictureTensor.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, td, vp, vp]
        L.H264SwDecNextPictureTensor.restype = i32
    if hasattr(L, "h264mi_tensor_colour_coeffs"):       # (optional, as above)
        L.h264mi_tensor_colour_coeffs.argtypes = [i32, C.POINTER(i32 * 6)]
        L.h264mi_tensor_colour_coeffs.restype = i32
        L.h264mi_tensor_colour_resolve.argtypes = [i32] * 5
        L.h264mi_tensor_colour_resolve.restype = i32
        L.H264SwDecLastTensorColour.argtypes = [vp]
        L.H264SwDecLastTensorColour.restype = i32
    if hasattr(L, "h264mi_tensor_resize_device_pitch"):     # (optional, as above)
        rd = C.POINTER(TensorResizeDesc)
        L.h264mi_tensor_resize_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, rd, vp, sz, vp]
        L.h264mi_tensor_resize_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_resized.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), rd, vp, sz, vp]
        L.h264mi_engine_export_tensor_resized.restype = i32
        L.H264SwDecNextPictureTensorResized.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, rd, vp, vp]
        L.H264SwDecNextPictureTensorResized.restype = i32
    if hasattr(L, "h264mi_tensor_rois_device_pitch"):       # (optional, as above)
        rd, ro = C.POINTER(TensorResizeDesc), C.POINTER(Roi)
        L.h264mi_tensor_rois_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, rd, ro, i32, vp, sz, vp]
        L.h264mi_tensor_rois_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_rois.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), rd, ro, i32, vp, sz, vp]
        L.h264mi_engine_export_tensor_rois.restype = i32
        L.H264SwDecLastPictureTensorRois.argtypes = [vp, rd, ro, u32, vp, vp]
        L.H264SwDecLastPictureTensorRois.restype = i32
    if hasattr(L, "h264mi_tensor_fit_device_pitch"):        # (optional, as above)
        fd, ro = C.POINTER(TensorFitDesc), C.POINTER(Roi)
        L.h264mi_letterbox_fit.argtypes = [i32, i32, i32, i32, i32, C.POINTER(i32)]
        L.h264mi_letterbox_fit.restype = i32
        L.h264mi_tensor_fit_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, fd, vp, sz, vp]
        L.h264mi_tensor_fit_device_pitch.restype = i32
        L.h264mi_tensor_rois_fit_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, fd, ro, i32, vp, sz, vp]
        L.h264mi_tensor_rois_fit_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_fit.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), fd, vp, sz, vp]
        L.h264mi_engine_export_tensor_fit.restype = i32
        L.h264mi_engine_export_tensor_rois_fit.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), fd, ro, i32, vp, sz, vp]
        L.h264mi_engine_export_tensor_rois_fit.restype = i32
        L.H264SwDecNextPictureTensorFit.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, fd, vp, vp]
        L.H264SwDecNextPictureTensorFit.restype = i32
        L.H264SwDecLastPictureTensorRoisFit.argtypes = [vp, fd, ro, u32, vp, vp]
        L.H264SwDecLastPictureTensorRoisFit.restype = i32
    if hasattr(L, "h264mi_tensor_layout_device_pitch"):     # (optional, as above)
        ld, ro = C.POINTER(TensorLayoutDesc), C.POINTER(Roi)
        L.h264mi_tensor_layout_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, ld, ro, i32, vp, sz, vp]
        L.h264mi_tensor_layout_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_layout.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), ld, ro, i32, vp, sz, vp]
        L.h264mi_engine_export_tensor_layout.restype = i32
        L.H264SwDecNextPictureTensorLayout.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, ld, vp, vp]
        L.H264SwDecNextPictureTensorLayout.restype = i32
        L.H264SwDecLastPictureTensorRoisLayout.argtypes = [vp, ld, ro, u32, vp, vp]
        L.H264SwDecLastPictureTensorRoisLayout.restype = i32
    if hasattr(L, "h264mi_tensor_warps_device_pitch"):      # (optional, as above)
        wd, wa = C.POINTER(TensorWarpDesc), C.POINTER(Warp)
        L.h264mi_tensor_warps_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, wd, wa, i32, vp, sz, vp]
        L.h264mi_tensor_warps_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_warps.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), wd, wa, i32, vp, sz, vp]
        L.h264mi_engine_export_tensor_warps.restype = i32
        L.H264SwDecLastPictureTensorWarps.argtypes = [vp, wd, wa, u32, vp, vp]
        L.H264SwDecLastPictureTensorWarps.restype = i32
    if hasattr(L, "h264mi_stats_device_pitch"):             # (optional, as above)
        sd, ro = C.POINTER(StatsDesc), C.POINTER(Roi)
        L.h264mi_stats_item_words.argtypes = [sd]
        L.h264mi_stats_item_words.restype = sz
        L.h264mi_stats_device_pitch.argtypes = [vp, C.POINTER(sz), vp, C.POINTER(sz), i32, i32, i32, i32, sd, ro, i32, vp,
                                                sz, vp]
        L.h264mi_stats_device_pitch.restype = i32
        L.h264mi_engine_export_stats.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                                 sd, ro, i32, vp, sz, vp]
        L.h264mi_engine_export_stats.restype = i32
        L.H264SwDecLastPictureStats.argtypes = [vp, sd, ro, u32, vp, vp]
        L.H264SwDecLastPictureStats.restype = i32
    if hasattr(L, "h264mi_tensor_dest_device_pitch"):       # (optional, as above)
        ld, ro, de = C.POINTER(TensorLayoutDesc), C.POINTER(Roi), C.POINTER(TensorDest)
        wd, wa = C.POINTER(TensorWarpDesc), C.POINTER(Warp)
        L.h264mi_tensor_dest_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, ld, ro, i32, de, vp, sz, vp]
        L.h264mi_tensor_dest_device_pitch.restype = i32
        L.h264mi_tensor_warps_dest_device_pitch.argtypes = [vp, C.POINTER(sz), i32, i32, i32, i32, wd, wa, i32, de, vp, sz,
                                                            vp]
        L.h264mi_tensor_warps_dest_device_pitch.restype = i32
        L.h264mi_engine_export_tensor_dest.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), ld, ro, i32, de, vp, sz, vp]
        L.h264mi_engine_export_tensor_dest.restype = i32
        L.h264mi_engine_export_tensor_warps_dest.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), wd, wa, i32, de, vp,
                                                             sz, vp]
        L.h264mi_engine_export_tensor_warps_dest.restype = i32
        L.H264SwDecNextPictureTensorDest.argtypes = [vp, C.POINTER(H264SwDecPicture), u32, ld, de, vp, vp]
        L.H264SwDecNextPictureTensorDest.restype = i32
    if hasattr(L, "h264mi_mbinfo_device"):                  # (optional, as above)
        md = C.POINTER(MbInfoDesc)
        L.h264mi_mbinfo_device.argtypes = [vp, C.POINTER(sz), i32, i32, i32, md, vp, sz, vp]
        L.h264mi_mbinfo_device.restype = i32
        L.h264mi_engine_keep_records.argtypes = [vp, i32]
        L.h264mi_engine_keep_records.restype = i32
        L.h264mi_engine_forget_records.argtypes = [vp, i32, i32]
        L.h264mi_engine_forget_records.restype = i32
        L.h264mi_engine_export_mbinfo.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), md, vp, sz, vp]
        L.h264mi_engine_export_mbinfo.restype = i32
        L.H264SwDecKeepMbInfo.argtypes = [vp, u32]
        L.H264SwDecKeepMbInfo.restype = i32
        L.H264SwDecLastPictureMbInfo.argtypes = [vp, md, vp, vp]
        L.H264SwDecLastPictureMbInfo.restype = i32
    if hasattr(L, "h264mi_residual_device"):                # (optional, as above)
        rs = C.POINTER(ResidualDesc)
        L.h264mi_residual_device.argtypes = [vp, C.POINTER(sz), vp, C.POINTER(u32), sz, i32, i32, i32, rs, vp, sz, vp]
        L.h264mi_residual_device.restype = i32
        L.h264mi_engine_keep_coefs.argtypes = [vp, i32]
        L.h264mi_engine_keep_coefs.restype = i32
        L.h264mi_engine_export_residual.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), rs, vp, sz, vp]
        L.h264mi_engine_export_residual.restype = i32
        L.H264SwDecKeepResidual.argtypes = [vp, u32]
        L.H264SwDecKeepResidual.restype = i32
        L.H264SwDecLastPictureResidual.argtypes = [vp, rs, vp, vp]
        L.H264SwDecLastPictureResidual.restype = i32
    if hasattr(L, "h264mi_accmv_device"):                   # (optional, as above)
        ad = C.POINTER(AccMvDesc)
        L.h264mi_accmv_step_device.argtypes = [vp, i32, i32, C.POINTER(vp), i32, i32, vp, vp]
        L.h264mi_accmv_step_device.restype = i32
        L.h264mi_accmv_device.argtypes = [vp, C.POINTER(sz), i32, i32, i32, ad, vp, sz, vp]
        L.h264mi_accmv_device.restype = i32
        L.h264mi_engine_keep_accmv.argtypes = [vp, i32]
        L.h264mi_engine_keep_accmv.restype = i32
        L.h264mi_engine_export_accmv.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), ad, vp, sz, vp]
        L.h264mi_engine_export_accmv.restype = i32
        L.H264SwDecKeepAccMotion.argtypes = [vp, u32]
        L.H264SwDecKeepAccMotion.restype = i32
        L.H264SwDecLastPictureAccMotion.argtypes = [vp, ad, vp, vp]
        L.H264SwDecLastPictureAccMotion.restype = i32
    if hasattr(L, "h264mi_accres_device"):                  # (optional, as above)
        rd = C.POINTER(AccResDesc)
        szp = C.POINTER(sz)
        L.h264mi_accres_device.argtypes = [vp, szp, vp, szp, vp, szp, i32, i32, i32, rd, vp, sz, vp]
        L.h264mi_accres_device.restype = i32
        L.h264mi_engine_keep_accres.argtypes = [vp, i32]
        L.h264mi_engine_keep_accres.restype = i32
        L.h264mi_engine_accres_held.argtypes = [vp, i32, i32]
        L.h264mi_engine_accres_held.restype = i32
        L.h264mi_engine_export_accres.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), rd, vp, sz, vp]
        L.h264mi_engine_export_accres.restype = i32
        L.h264mi_engine_conceal.argtypes = [vp, i32, i32, C.POINTER(i32), i32, C.POINTER(C.c_uint8)]
        L.h264mi_engine_conceal.restype = i32
    if hasattr(L, "h264mi_accmv_resize_device"):            # (optional, as above)
        ad, rd = C.POINTER(AccMvResizeDesc), C.POINTER(AccResResizeDesc)
        szp = C.POINTER(sz)
        L.h264mi_accmv_resize_device.argtypes = [vp, szp, i32, i32, i32, ad, vp, sz, vp]
        L.h264mi_accmv_resize_device.restype = i32
        L.h264mi_accres_resize_device.argtypes = [vp, szp, vp, szp, vp, szp, i32, i32, i32, rd, vp, sz, vp]
        L.h264mi_accres_resize_device.restype = i32
        L.h264mi_engine_export_accmv_resized.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), ad, vp, sz, vp]
        L.h264mi_engine_export_accmv_resized.restype = i32
        L.h264mi_engine_export_accres_resized.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), rd, vp, sz, vp]
        L.h264mi_engine_export_accres_resized.restype = i32
        L.H264SwDecLastPictureAccMotionResized.argtypes = [vp, ad, vp, vp]
        L.H264SwDecLastPictureAccMotionResized.restype = i32
    L.h264mi_engine_sync.argtypes = [vp]
    L.h264mi_engine_sync.restype = i32
    L.h264mi_engine_kernel.argtypes = [vp]
    L.h264mi_engine_kernel.restype = C.c_char_p
    L.h264mi_engine_errors.argtypes = [vp]
    L.h264mi_engine_errors.restype = u32
    L.h264mi_engine_rows_per_workgroup.argtypes = [vp, C.c_int]
    L.h264mi_engine_rows_per_workgroup.restype = C.c_int
    L.h264mi_engine_last_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.h264mi_engine_last_timing.restype = i32
    L.h264mi_engine_set_timing.argtypes = [vp, i32]
    L.h264mi_engine_set_timing.restype = i32
    L.h264mi_engine_set_timing_stride.argtypes = [vp, i32]
    L.h264mi_engine_set_timing_stride.restype = i32
    L.h264mi_engine_timing_report.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32)]
    L.h264mi_engine_timing_report.restype = i32
    # (round-4 additions; absent from older builds loaded for A/B timing)
    if hasattr(L, "h264mi_engine_error_bits"):
        L.h264mi_engine_error_bits.argtypes = [vp]
        L.h264mi_engine_error_bits.restype = C.c_uint32
    if hasattr(L, "h264mi_engine_timing_list"):
        L.h264mi_engine_timing_list.argtypes = [vp, C.POINTER(C.c_double), i32]
        L.h264mi_engine_timing_list.restype = i32
    L.h264mi_engine_profile.argtypes = [vp, i32, C.POINTER(C.c_uint64), sz]
    L.h264mi_engine_profile.restype = i32
    L.h264mi_engine_frame_ptr.argtypes = [vp, i32, i32]
    L.h264mi_engine_frame_ptr.restype = vp
    L.h264mi_engine_frame_bytes.argtypes = [vp]
    L.h264mi_engine_frame_bytes.restype = sz
    if hasattr(L, "h264mi_engine_slot_bytes"):
        L.h264mi_engine_slot_bytes.argtypes = [vp]
        L.h264mi_engine_slot_bytes.restype = sz
        L.h264mi_engine_chroma_pitch.argtypes = [vp]
        L.h264mi_engine_chroma_pitch.restype = i32
    L.h264mi_capture_stream.argtypes = [vp, sz, i32]
    L.h264mi_capture_stream.restype = vp
    L.h264mi_capture_info.argtypes = [vp] + [C.POINTER(i32)] * 5
    L.h264mi_capture_info.restype = i32
    L.h264mi_capture_picture.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u32),
                                         C.POINTER(i32), C.POINTER(C.c_uint64)]
    L.h264mi_capture_picture.restype = i32
    L.h264mi_capture_stats.argtypes = [vp, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.h264mi_capture_stats.restype = i32
    L.h264mi_capture_ref_lines.argtypes = [vp, i32, C.POINTER(C.c_uint64)]
    L.h264mi_capture_ref_lines.restype = i32
    L.h264mi_capture_free.argtypes = [vp]
    L.h264mi_capture_free.restype = None
    L.h264mi_device_alloc.argtypes = [sz]
    L.h264mi_device_alloc.restype = vp
    L.h264mi_device_free.argtypes = [vp]
    L.h264mi_device_free.restype = i32
    L.h264mi_copy_h2d.argtypes = [vp, vp, sz]
    L.h264mi_copy_h2d.restype = i32
    L.h264mi_engine_device.argtypes = [vp]
    L.h264mi_engine_device.restype = i32
    L.h264mi_engine_alloc.argtypes = [vp, sz]
    L.h264mi_engine_alloc.restype = vp
    L.h264mi_engine_free.argtypes = [vp, vp]
    L.h264mi_engine_free.restype = i32
    L.h264mi_engine_copy_h2d.argtypes = [vp, vp, vp, sz]
    L.h264mi_engine_copy_h2d.restype = i32
    L.h264mi_pointer_device.argtypes = [vp]
    L.h264mi_pointer_device.restype = i32
    _mi = L
    return L


def gen() -> C.CDLL:
    global _gen
    if _gen is not None:
        return _gen
    L = _load("libh264gen.so")
    L.h264gen_default_params.argtypes = [C.POINTER(GenParams), C.c_int, C.c_int]
    L.h264gen_default_params.restype = None
    L.h264gen_preset.argtypes = [C.POINTER(GenParams), C.c_int, C.c_uint64]
    L.h264gen_preset.restype = C.c_int
    L.h264gen_generate.argtypes = [C.POINTER(GenParams), C.POINTER(C.POINTER(C.c_uint8)),
                                   C.POINTER(C.c_size_t)]
    L.h264gen_generate.restype = C.c_int
    L.h264gen_free.argtypes = [C.c_void_p]
    L.h264gen_free.restype = None
    L.h264gen_cavlc_selftest.argtypes = [C.c_int, C.c_uint64]
    L.h264gen_cavlc_selftest.restype = C.c_int
    _gen = L
    return L
