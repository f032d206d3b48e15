"""ctypes binding of libheadtrackr_hip.so (include/headtrackr_hip.h) — the only compute path of this package.

There is deliberately no CPU fallback: if the shared library is missing or no gfx950 device is visible, importing
`lib()` / creating a context raises.  (The CPU checker lives in oracle/ and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HEADTRACKR_HIP_LIB: load another BUILD of the same library (an instrumented variant from tools/build_alt.py) — a loader path like
# LD_LIBRARY_PATH, not a behaviour switch: the library itself reads no environment variable
LIB_PATH = os.environ.get("HEADTRACKR_HIP_LIB") or os.path.join(_HERE, "libheadtrackr_hip.so")

HT_OK = 0
HT_ERR_CAPACITY = -4
HT_INPUT_RGBA = 0
HT_INPUT_GRAY_IN_R = 1
HT_SCAN_NO_SPLIT = 2
HT_SCAN_SIMPLE = 4
HT_SCAN_GENERIC = 8
HT_SCAN_STATS = 16
HT_DETECT_WHITEBALANCE = 32
HT_MAX_LEVELS = 96
HT_BP_RGBA8 = 0  # ht_camshift_backproject kinds: 4 bytes (v, v, v, 255) per pixel ...
HT_BP_F64 = 1    # ... or one binary64 (the pdf) per pixel
HT_ERR_INVALID = -1
HT_ERR_STATE = -6
# ht_camshift_init_best's decision per pair
HT_CSB_UNTOUCHED, HT_CSB_FACE, HT_CSB_FALLBACK, HT_CSB_DEFERRED = 0, 1, 2, 3
# ht_camshift_init_faces: its flag, the slots one frame may have in a call
HT_CSF_ASSOCIATE = 1
HT_CSF_MAX_SLOTS = 16


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("interval", C.c_int32),
        ("hit_capacity", C.c_uint32),
        ("stream", C.c_void_p),
        ("queue_capacity", C.c_uint32),
        ("flags", C.c_uint32),
        ("options", C.c_char_p),  # "key=value,...": per-context schedule selectors (include/headtrackr_hip.h); None = defaults
    ]


HIT_DTYPE = np.dtype(
    [("frame", "<u4"), ("x", "<u2"), ("y", "<u2"), ("scale", "u1"), ("q", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4"), ("sum", "<f8")]
)
RECT_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("width", "<f8"), ("height", "<f8"), ("confidence", "<f8"), ("neighbors", "<i4"), ("reserved", "<i4")]
)
CS_RECT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4")])
# ht_csf_record (ht_camshift_init_faces_result), 32 bytes
CSF_RECORD_DTYPE = np.dtype([("code", "<i4"), ("face", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("dropped", "<i4"), ("reserved", "<i4")])
PAIR_DTYPE = np.dtype([("stream", "<i4"), ("frame", "<i4")])  # ht_cs_pair: tracker `stream` meets bound frame `frame`
CS_TRACKOBJ_DTYPE = np.dtype(
    [("x", "<f8"), ("y", "<f8"), ("width", "<f8"), ("height", "<f8"), ("angle", "<f8"),
     ("sw_x", "<i4"), ("sw_y", "<i4"), ("sw_width", "<i4"), ("sw_height", "<i4")]
)
KERNEL_TIME_DTYPE = np.dtype([("name", "S32"), ("ms", "<f8"), ("launches", "<u4"), ("reserved", "<u4")])
assert HIT_DTYPE.itemsize == 24 and RECT_DTYPE.itemsize == 48 and CS_TRACKOBJ_DTYPE.itemsize == 56 and KERNEL_TIME_DTYPE.itemsize == 48


class PlaneInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("present", C.c_int32), ("offset", C.c_uint64)]


class YUV_FRAMES(C.Structure):
    """ht_yuv_frames: n YUV 4:2:0 frames in device memory (ht_draw_frames_yuv_device)"""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_pitch", C.c_size_t), ("c_pitch", C.c_size_t), ("frame_stride", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32), ("matrix", C.c_int32)]


class CS_RECT(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class DRAW_SOURCE(C.Structure):
    """ht_draw_source: one entry of ht_draw_list_device — a source with an allocation, size, format, matrix and rect of its own"""
    _fields_ = [("p0", C.c_void_p), ("p1", C.c_void_p), ("p2", C.c_void_p), ("pitch0", C.c_size_t), ("pitch1", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32), ("format", C.c_int32), ("matrix", C.c_int32), ("rect", CS_RECT)]


class CROP_PARAMS(C.Structure):
    """ht_crop_params: patch size, margin in 1/256 and flags of a crop call"""
    _fields_ = [("out_width", C.c_int32), ("out_height", C.c_int32), ("margin_q8", C.c_int32), ("flags", C.c_uint32)]


class CROP_RECORD(C.Structure):
    """ht_crop_record: what a crop call decided for one entry"""
    _fields_ = [("code", C.c_int32), ("stream", C.c_int32), ("rect", CS_RECT), ("rx", C.c_double), ("ry", C.c_double)]


CROP_RECORD_DTYPE = np.dtype([("code", "<i4"), ("stream", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("rx", "<f8"), ("ry", "<f8")])
assert C.sizeof(CROP_RECORD) == CROP_RECORD_DTYPE.itemsize == 40 and C.sizeof(CROP_PARAMS) == 16
HT_CROP_EMPTY, HT_CROP_FACE = 0, 1
HT_CROP_SQUARE = 1


class ALIGN_PARAMS(C.Structure):
    """ht_align_params: patch size, margin in 1/256 and flags of an align call"""
    _fields_ = [("out_width", C.c_int32), ("out_height", C.c_int32), ("margin_q8", C.c_int32), ("flags", C.c_uint32)]


class ALIGN_RECORD(C.Structure):
    """ht_align_record: what an align call decided for one entry (centre and the patch's two vectors in Q16 source pixels)"""
    _fields_ = [("code", C.c_int32), ("stream", C.c_int32), ("a12", C.c_int32), ("pad", C.c_int32), ("cx", C.c_int64), ("cy", C.c_int64), ("ux", C.c_int64),
                ("uy", C.c_int64), ("vx", C.c_int64), ("vy", C.c_int64)]


ALIGN_RECORD_DTYPE = np.dtype([("code", "<i4"), ("stream", "<i4"), ("a12", "<i4"), ("pad", "<i4"), ("cx", "<i8"), ("cy", "<i8"), ("ux", "<i8"), ("uy", "<i8"), ("vx", "<i8"),
                               ("vy", "<i8")])
assert C.sizeof(ALIGN_RECORD) == ALIGN_RECORD_DTYPE.itemsize == 64 and C.sizeof(ALIGN_PARAMS) == 16
HT_ALIGN_EMPTY, HT_ALIGN_FACE = 0, 1
HT_ALIGN_SQUARE = 1


class PATCH_FORMAT(C.Structure):
    """ht_patch_format: dtype, layout, channel order and per-channel normalisation of a tensor call's output"""
    _fields_ = [("dtype", C.c_int32), ("layout", C.c_int32), ("channels", C.c_int32), ("pad", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


assert C.sizeof(PATCH_FORMAT) == 40
HT_PATCH_F32, HT_PATCH_F16, HT_PATCH_BF16 = 0, 1, 2
HT_PATCH_CHW, HT_PATCH_HWC = 0, 1
HT_PATCH_RGB, HT_PATCH_BGR, HT_PATCH_GRAY = 0, 1, 2
PATCH_DTYPES = {"f32": HT_PATCH_F32, "f16": HT_PATCH_F16, "bf16": HT_PATCH_BF16}
PATCH_LAYOUTS = {"chw": HT_PATCH_CHW, "hwc": HT_PATCH_HWC}
PATCH_CHANNELS = {"rgb": HT_PATCH_RGB, "bgr": HT_PATCH_BGR, "gray": HT_PATCH_GRAY}

HT_FILTER_MAX_FACTOR = 8  # the largest max_factor of the _filtered calls

HT_YUV_NV12, HT_YUV_I420 = 0, 1
HT_YUV_YUYV, HT_YUV_UYVY = 4, 5  # packed 4:2:2: one plane of 4-byte macropixels (2, 3, 6 are no formats)
HT_DRAW_RGBA = 16  # ht_draw_source.format beside the four above (no format of the YUV entry points)
HT_YUV_BT601_LIMITED, HT_YUV_BT709_LIMITED, HT_YUV_BT601_FULL, HT_YUV_BT709_FULL = 0, 1, 2, 3
YUV_FORMATS = {"nv12": HT_YUV_NV12, "i420": HT_YUV_I420, "yuyv": HT_YUV_YUYV, "uyvy": HT_YUV_UYVY}
YUV_PACKED_422 = (HT_YUV_YUYV, HT_YUV_UYVY)
DRAW_FORMATS = {"nv12": HT_YUV_NV12, "i420": HT_YUV_I420, "rgba": HT_DRAW_RGBA}  # the entry formats before packed 4:2:2 (tests/test_draw_list_cpu.py holds this table to these three)
DRAW_LIST_FORMATS = dict(DRAW_FORMATS, yuyv=HT_YUV_YUYV, uyvy=HT_YUV_UYVY)  # what an ht_draw_source entry may be: api.py reads THIS table
YUV_MATRICES = {"bt601": HT_YUV_BT601_LIMITED, "bt709": HT_YUV_BT709_LIMITED, "bt601-full": HT_YUV_BT601_FULL, "bt709-full": HT_YUV_BT709_FULL}

# every symbol include/headtrackr_hip.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = [
    "ht_create", "ht_destroy", "ht_last_error", "ht_abi_version", "ht_set_geometry", "ht_num_levels", "ht_plane",
    "ht_windows_per_frame", "ht_pyramid_bytes_per_frame", "ht_upload_frames", "ht_upload_frames_async", "ht_swap_frames", "ht_bind_frames_device", "ht_frames_bound", "ht_frames_enqueued", "ht_host_alloc", "ht_host_free", "ht_device_alloc", "ht_device_free", "ht_device_upload", "ht_device_download", "ht_draw_frames_device", "ht_draw_frames", "ht_draw_frames_yuv_device", "ht_draw_frames_yuv", "ht_draw_list_device", "ht_draw_list_filtered_device", "ht_draw_filter_factors", "ht_detect_enqueue",
    "ht_detect_collect", "ht_detect_batch", "ht_pyramid_readback", "ht_stage_counts", "ht_grayscale_batch",
    "ht_whitebalance_batch", "ht_detect_whitebalance", "ht_hits_to_rects", "ht_group_rects", "ht_best_faces", "ht_detect_collect_best", "ht_detect_collect_best_requeue", "ht_detect_best_enqueue", "ht_detect_best_collect", "ht_detect_best_collect_requeue", "ht_detect_grouped", "ht_detect_best_records_device", "ht_group_hits", "ht_camshift_reserve", "ht_camshift_init_batch",
    "ht_camshift_track_batch", "ht_camshift_track_collect", "ht_camshift_init_pairs", "ht_camshift_track_pairs", "ht_camshift_init_best", "ht_camshift_init_best_result", "ht_camshift_init_faces", "ht_camshift_init_faces_result", "ht_camshift_track_sequence", "ht_camshift_sequence_collect", "ht_camshift_stats", "ht_camshift_debug_hist", "ht_camshift_backproject", "ht_camshift_backproject_device", "ht_camshift_backproject_pairs", "ht_camshift_backproject_pairs_device", "ht_camshift_crop_pairs_device", "ht_camshift_crop_sources_device", "ht_camshift_crop_result", "ht_camshift_crop_records_device", "ht_camshift_align_pairs_device", "ht_camshift_align_sources_device", "ht_camshift_align_result", "ht_camshift_align_records_device", "ht_camshift_crop_pairs_tensor_device", "ht_camshift_crop_sources_tensor_device", "ht_camshift_align_pairs_tensor_device", "ht_camshift_align_sources_tensor_device", "ht_camshift_crop_pairs_filtered_device", "ht_camshift_crop_sources_filtered_device", "ht_camshift_align_pairs_filtered_device", "ht_camshift_align_sources_filtered_device", "ht_camshift_crop_filter_factors", "ht_camshift_align_filter_factors", "ht_allgather_records", "ht_allgather_best_faces", "ht_device_count", "ht_profile", "ht_kernel_times", "ht_stream", "ht_graph_launches", "ht_synchronize",
]

_lib = None


def lib():
    """Loads libheadtrackr_hip.so; raises if it has not been built (python -m headtrackr_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m headtrackr_amd.build` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    vp, u8p, i32, u32, sz = C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
    L.ht_create.restype = i32
    L.ht_create.argtypes = [C.POINTER(Config), vp, sz, C.POINTER(vp)]
    L.ht_destroy.restype = None
    L.ht_destroy.argtypes = [vp]
    L.ht_last_error.restype = C.c_char_p
    L.ht_last_error.argtypes = [vp]
    L.ht_abi_version.restype = i32
    L.ht_set_geometry.restype = i32
    L.ht_set_geometry.argtypes = [vp, i32, i32, i32, vp, i32]
    L.ht_num_levels.restype = i32
    L.ht_num_levels.argtypes = [vp]
    L.ht_plane.restype = i32
    L.ht_plane.argtypes = [vp, i32, i32, C.POINTER(PlaneInfo)]
    L.ht_windows_per_frame.restype = C.c_uint64
    L.ht_windows_per_frame.argtypes = [vp]
    L.ht_pyramid_bytes_per_frame.restype = C.c_uint64
    L.ht_pyramid_bytes_per_frame.argtypes = [vp]
    L.ht_upload_frames.restype = i32
    L.ht_upload_frames.argtypes = [vp, u8p, i32, sz]
    L.ht_upload_frames_async.restype = i32
    L.ht_upload_frames_async.argtypes = [vp, u8p, i32, sz]
    L.ht_swap_frames.restype = i32
    L.ht_swap_frames.argtypes = [vp]
    L.ht_bind_frames_device.restype = i32
    L.ht_bind_frames_device.argtypes = [vp, vp, i32, sz]
    L.ht_frames_bound.restype = i32
    L.ht_frames_bound.argtypes = [vp]
    L.ht_frames_enqueued.restype = i32
    L.ht_frames_enqueued.argtypes = [vp]
    L.ht_host_alloc.restype = i32
    L.ht_host_alloc.argtypes = [sz, C.POINTER(vp)]
    L.ht_host_free.restype = None
    L.ht_host_free.argtypes = [vp]
    L.ht_device_alloc.restype = i32
    L.ht_device_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.ht_device_free.restype = i32
    L.ht_device_free.argtypes = [vp, vp]
    L.ht_device_upload.restype = i32
    L.ht_device_upload.argtypes = [vp, vp, vp, sz]
    L.ht_device_download.restype = i32
    L.ht_device_download.argtypes = [vp, vp, vp, sz]
    L.ht_draw_frames_device.restype = i32
    L.ht_draw_frames_device.argtypes = [vp, vp, i32, i32, i32, sz, sz, vp, vp, sz]
    L.ht_draw_frames.restype = i32
    L.ht_draw_frames.argtypes = [vp, u8p, i32, i32, i32, sz, vp]
    L.ht_draw_frames_yuv_device.restype = i32
    L.ht_draw_frames_yuv_device.argtypes = [vp, C.POINTER(YUV_FRAMES), i32, vp, vp, sz]
    L.ht_draw_frames_yuv.restype = i32
    L.ht_draw_frames_yuv.argtypes = [vp, u8p, i32, i32, i32, i32, i32, sz, vp]
    L.ht_draw_list_device.restype = i32
    L.ht_draw_list_device.argtypes = [vp, C.POINTER(DRAW_SOURCE), i32, vp, sz]
    L.ht_draw_list_filtered_device.restype = i32
    L.ht_draw_list_filtered_device.argtypes = [vp, C.POINTER(DRAW_SOURCE), i32, i32, vp, sz]
    L.ht_draw_filter_factors.restype = i32
    L.ht_draw_filter_factors.argtypes = [i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ht_detect_enqueue.restype = i32
    L.ht_detect_enqueue.argtypes = [vp, u32]
    L.ht_detect_collect.restype = i32
    L.ht_detect_collect.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
    L.ht_detect_batch.restype = i32
    L.ht_detect_batch.argtypes = [vp, u8p, i32, i32, i32, sz, u32, vp, u32, vp, C.POINTER(u32)]
    L.ht_pyramid_readback.restype = i32
    L.ht_pyramid_readback.argtypes = [vp, i32, i32, i32, u8p, sz]
    L.ht_stage_counts.restype = i32
    L.ht_stage_counts.argtypes = [vp, vp, i32]
    L.ht_grayscale_batch.restype = i32
    L.ht_grayscale_batch.argtypes = [vp, u8p, i32, i32, i32, sz]
    L.ht_whitebalance_batch.restype = i32
    L.ht_whitebalance_batch.argtypes = [vp, vp, i32]
    L.ht_hits_to_rects.restype = i32
    L.ht_hits_to_rects.argtypes = [vp, vp, u32, vp]
    L.ht_group_rects.restype = i32
    L.ht_group_rects.argtypes = [vp, u32, i32, vp, C.POINTER(u32)]
    L.ht_best_faces.restype = i32
    L.ht_best_faces.argtypes = [vp, vp, vp, i32, i32, vp]
    L.ht_detect_collect_best.restype = i32
    L.ht_detect_collect_best.argtypes = [vp, i32, vp, C.POINTER(u32)]
    L.ht_detect_collect_best_requeue.restype = i32
    L.ht_detect_collect_best_requeue.argtypes = [vp, i32, vp, vp, C.c_uint32]
    L.ht_detect_best_enqueue.restype = i32
    L.ht_detect_best_enqueue.argtypes = [vp, i32, i32]
    L.ht_detect_best_collect.restype = i32
    L.ht_detect_best_collect.argtypes = [vp, vp, C.POINTER(u32)]
    L.ht_detect_best_collect_requeue.restype = i32
    L.ht_detect_best_collect_requeue.argtypes = [vp, vp, C.POINTER(u32), u32]
    L.ht_detect_grouped.restype = i32
    L.ht_detect_grouped.argtypes = [vp, i32, vp, u32, C.POINTER(u32)]
    L.ht_detect_best_records_device.restype = i32
    L.ht_detect_best_records_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    L.ht_group_hits.restype = i32
    L.ht_group_hits.argtypes = [vp, vp, u32, i32, i32, vp, vp, vp]
    L.ht_camshift_reserve.restype = i32
    L.ht_camshift_reserve.argtypes = [vp, i32]
    L.ht_camshift_init_batch.restype = i32
    L.ht_camshift_init_batch.argtypes = [vp, i32, i32, vp]
    L.ht_camshift_track_batch.restype = i32
    L.ht_camshift_track_batch.argtypes = [vp, i32, i32, i32, vp]
    L.ht_camshift_init_pairs.restype = i32
    L.ht_camshift_init_pairs.argtypes = [vp, vp, i32, vp]
    L.ht_camshift_track_pairs.restype = i32
    L.ht_camshift_track_pairs.argtypes = [vp, vp, i32, i32, vp]
    L.ht_camshift_init_best.restype = i32
    L.ht_camshift_init_best.argtypes = [vp, vp, i32, C.c_double, vp]
    L.ht_camshift_init_best_result.restype = i32
    L.ht_camshift_init_best_result.argtypes = [vp, i32, vp, vp]
    L.ht_camshift_init_faces.restype = i32
    L.ht_camshift_init_faces.argtypes = [vp, vp, i32, C.c_double, C.c_uint32]
    L.ht_camshift_init_faces_result.restype = i32
    L.ht_camshift_init_faces_result.argtypes = [vp, i32, vp]
    L.ht_detect_whitebalance.restype = i32
    L.ht_detect_whitebalance.argtypes = [vp, vp, i32]
    L.ht_camshift_track_sequence.restype = i32
    L.ht_camshift_track_sequence.argtypes = [vp, i32, i32, i32, vp, i32, sz, vp, i32]
    L.ht_camshift_sequence_collect.restype = i32
    L.ht_camshift_sequence_collect.argtypes = [vp, i32, i32, i32, vp]
    L.ht_camshift_stats.restype = i32
    L.ht_camshift_stats.argtypes = [vp, i32, i32, vp, vp, i32]
    L.ht_camshift_debug_hist.restype = i32
    L.ht_camshift_debug_hist.argtypes = [vp, i32, vp, vp]
    L.ht_camshift_backproject.restype = i32
    L.ht_camshift_backproject.argtypes = [vp, i32, i32, i32, vp, sz]
    L.ht_camshift_backproject_device.restype = i32
    L.ht_camshift_backproject_device.argtypes = [vp, i32, i32, i32, vp, sz]
    L.ht_camshift_backproject_pairs.restype = i32
    L.ht_camshift_backproject_pairs.argtypes = [vp, vp, i32, i32, vp, sz]
    L.ht_camshift_backproject_pairs_device.restype = i32
    L.ht_camshift_backproject_pairs_device.argtypes = [vp, vp, i32, i32, vp, sz]
    L.ht_camshift_crop_pairs_device.restype = i32
    L.ht_camshift_crop_pairs_device.argtypes = [vp, vp, i32, C.POINTER(CROP_PARAMS), vp, sz]
    L.ht_camshift_crop_sources_device.restype = i32
    L.ht_camshift_crop_sources_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(CROP_PARAMS), vp, sz]
    L.ht_camshift_crop_result.restype = i32
    L.ht_camshift_crop_result.argtypes = [vp, i32, vp]
    L.ht_camshift_crop_records_device.restype = i32
    L.ht_camshift_crop_records_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    L.ht_camshift_align_pairs_device.restype = i32
    L.ht_camshift_align_pairs_device.argtypes = [vp, vp, i32, C.POINTER(ALIGN_PARAMS), vp, sz]
    L.ht_camshift_align_sources_device.restype = i32
    L.ht_camshift_align_sources_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(ALIGN_PARAMS), vp, sz]
    L.ht_camshift_align_result.restype = i32
    L.ht_camshift_align_result.argtypes = [vp, i32, vp]
    L.ht_camshift_align_records_device.restype = i32
    L.ht_camshift_align_records_device.argtypes = [vp, C.POINTER(vp), C.POINTER(i32)]
    L.ht_camshift_crop_pairs_tensor_device.restype = i32
    L.ht_camshift_crop_pairs_tensor_device.argtypes = [vp, vp, i32, C.POINTER(CROP_PARAMS), C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_crop_sources_tensor_device.restype = i32
    L.ht_camshift_crop_sources_tensor_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(CROP_PARAMS), C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_align_pairs_tensor_device.restype = i32
    L.ht_camshift_align_pairs_tensor_device.argtypes = [vp, vp, i32, C.POINTER(ALIGN_PARAMS), C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_align_sources_tensor_device.restype = i32
    L.ht_camshift_align_sources_tensor_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(ALIGN_PARAMS), C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_crop_pairs_filtered_device.restype = i32
    L.ht_camshift_crop_pairs_filtered_device.argtypes = [vp, vp, i32, C.POINTER(CROP_PARAMS), i32, C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_crop_sources_filtered_device.restype = i32
    L.ht_camshift_crop_sources_filtered_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(CROP_PARAMS), i32, C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_align_pairs_filtered_device.restype = i32
    L.ht_camshift_align_pairs_filtered_device.argtypes = [vp, vp, i32, C.POINTER(ALIGN_PARAMS), i32, C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_align_sources_filtered_device.restype = i32
    L.ht_camshift_align_sources_filtered_device.argtypes = [vp, vp, C.POINTER(DRAW_SOURCE), i32, C.POINTER(ALIGN_PARAMS), i32, C.POINTER(PATCH_FORMAT), vp, sz]
    L.ht_camshift_crop_filter_factors.restype = i32
    L.ht_camshift_crop_filter_factors.argtypes = [vp, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ht_camshift_align_filter_factors.restype = i32
    L.ht_camshift_align_filter_factors.argtypes = [vp, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.ht_allgather_records.restype = i32
    L.ht_allgather_records.argtypes = [vp, i32, vp, sz]
    L.ht_allgather_best_faces.restype = i32
    L.ht_allgather_best_faces.argtypes = [vp, i32, vp, i32, vp]
    L.ht_device_count.restype = i32
    L.ht_device_count.argtypes = []
    L.ht_profile.restype = i32
    L.ht_profile.argtypes = [vp, i32]
    L.ht_kernel_times.restype = i32
    L.ht_kernel_times.argtypes = [vp, vp, C.POINTER(i32), i32]
    L.ht_stream.restype = vp
    L.ht_stream.argtypes = [vp]
    L.ht_camshift_track_collect.restype = i32
    L.ht_camshift_track_collect.argtypes = [vp, i32, vp]
    L.ht_graph_launches.restype = C.c_uint64
    L.ht_graph_launches.argtypes = [vp]
    L.ht_synchronize.restype = i32
    L.ht_synchronize.argtypes = [vp]
    _lib = L
    return L


class HtError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"headtrackr_hip status {status}: {msg}")
        self.status = status
