"""ctypes binding of liblitepi_hip.so (C-ABI: include/litepi.h).

The product path has no CPU fallback: if the library is missing or no gfx950 device is
usable, loading / ``lp_create`` fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblitepi_hip.so")

LP_FP32, LP_FP16 = 0, 1
LP_OK, LP_ERR_ARG, LP_ERR_IO, LP_ERR_GRAPH, LP_ERR_HIP, LP_ERR_STATE, LP_ERR_NODEVICE = 0, -1, -2, -3, -4, -5, -6


class LpConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("precision", C.c_int), ("max_batch", C.c_int), ("max_det", C.c_int),
                ("num_classes", C.c_int), ("det_input", C.c_int), ("cls_input", C.c_int), ("max_rois", C.c_int),
                ("conv_impl", C.c_int), ("numerics", C.c_int), ("cls_arch", C.c_int), ("det_input_h", C.c_int), ("reserved", C.c_int * 4)]


class LpDet(C.Structure):
    _fields_ = [("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float), ("det_conf", C.c_float),
                ("det_class", C.c_int32), ("cls_class", C.c_int32), ("cls_conf", C.c_float)]


class LpTiming(C.Structure):
    _fields_ = [("t_detection", C.c_float), ("t_roi_extract", C.c_float), ("t_classification", C.c_float),
                ("t_total", C.c_float)]


class LpKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("layer", C.c_char * 32), ("ms", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double)]


class LpTiling(C.Structure):
    _fields_ = [("overlap", C.c_int), ("full_frame", C.c_int), ("reserved", C.c_int * 6)]


class LpViewMerge(C.Structure):
    _fields_ = [("metric", C.c_int), ("mode", C.c_int), ("threshold", C.c_float), ("reserved", C.c_int * 5)]


LP_MATCH_IOU, LP_MATCH_IOS = 0, 1
LP_MERGE_SUPPRESS, LP_MERGE_UNION = 0, 1
LP_PIX_BGR8, LP_PIX_NV12 = 0, 1
LP_CSC_BT601_LIMITED, LP_CSC_BT709_LIMITED = 0, 1


class LpFrameFormat(C.Structure):
    _fields_ = [("pixfmt", C.c_int), ("matrix", C.c_int), ("pitch", C.c_int), ("reserved0", C.c_int), ("uv_offset", C.c_int64),
                ("frame_stride", C.c_int64), ("reserved", C.c_int * 6)]


LP_SURF_NV12, LP_SURF_P010 = 1, 2


class LpSurface(C.Structure):
    _fields_ = [("plane", C.c_void_p * 2), ("pitch", C.c_int * 2), ("height", C.c_int), ("width", C.c_int), ("reserved", C.c_int * 4)]


class LpSurfaceFormat(C.Structure):
    _fields_ = [("pixfmt", C.c_int), ("matrix", C.c_int), ("reserved", C.c_int * 6)]


class LpTrackConfig(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("max_tracks", C.c_int), ("iou_match", C.c_float), ("max_age", C.c_int),
                ("min_hits", C.c_int), ("new_conf", C.c_float), ("vote_decay", C.c_float), ("class_gate", C.c_int),
                ("motion", C.c_int), ("reserved", C.c_int * 7)]


class LpTrack(C.Structure):
    _fields_ = [("track_id", C.c_int32), ("slot", C.c_int32), ("hits", C.c_int32), ("age", C.c_int32), ("voted_class", C.c_int32),
                ("voted_conf", C.c_float), ("vote_weight", C.c_float), ("flags", C.c_int32)]


class LpTrackState(C.Structure):
    _fields_ = [("slot", C.c_int32), ("track_id", C.c_int32), ("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float),
                ("vx1", C.c_float), ("vy1", C.c_float), ("vx2", C.c_float), ("vy2", C.c_float), ("hits", C.c_int32),
                ("missed", C.c_int32), ("age", C.c_int32), ("det_class", C.c_int32), ("wsum", C.c_float), ("has_vote", C.c_int32)]


LP_TRACK_CONFIRMED, LP_TRACK_BORN = 1, 2


class LpInventoryConfig(C.Structure):
    _fields_ = [("max_signs", C.c_int), ("keep_crops", C.c_int), ("best", C.c_int), ("min_hits", C.c_int), ("reserved", C.c_int * 12)]


class LpSign(C.Structure):
    _fields_ = [("stream", C.c_int32), ("track_id", C.c_int32), ("first_frame", C.c_int32), ("last_frame", C.c_int32), ("hits", C.c_int32),
                ("voted_class", C.c_int32), ("voted_conf", C.c_float), ("vote_weight", C.c_float), ("best_frame", C.c_int32),
                ("best_quality", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float),
                ("det_class", C.c_int32), ("flags", C.c_int32)]


class LpEvidenceConfig(C.Structure):
    _fields_ = [("size", C.c_int), ("scale", C.c_float), ("reserved", C.c_int * 6)]


class LpFocusConfig(C.Structure):
    _fields_ = [("slots", C.c_int), ("side_min", C.c_int), ("side_max", C.c_int), ("margin", C.c_float), ("small_px", C.c_float),
                ("border", C.c_int), ("sweep", C.c_int), ("sweep_overlap", C.c_int), ("reserved", C.c_int * 8)]


LP_BEST_AREA, LP_BEST_DET_CONF, LP_BEST_CLS_CONF = 0, 1, 2
LP_SIGN_HAS_CROP, LP_SIGN_FLUSHED, LP_SIGN_HAS_EVIDENCE = 1, 2, 4
# numpy view of lp_sign records
SIGN_DTYPE = [("stream", "<i4"), ("track_id", "<i4"), ("first_frame", "<i4"), ("last_frame", "<i4"), ("hits", "<i4"), ("voted_class", "<i4"),
              ("voted_conf", "<f4"), ("vote_weight", "<f4"), ("best_frame", "<i4"), ("best_quality", "<f4"), ("x1", "<f4"), ("y1", "<f4"),
              ("x2", "<f4"), ("y2", "<f4"), ("det_class", "<i4"), ("flags", "<i4")]
# numpy views of lp_track records and of lp_track_state
TRACK_DTYPE = [("track_id", "<i4"), ("slot", "<i4"), ("hits", "<i4"), ("age", "<i4"), ("voted_class", "<i4"), ("voted_conf", "<f4"),
               ("vote_weight", "<f4"), ("flags", "<i4")]
TRACK_STATE_DTYPE = [("slot", "<i4"), ("track_id", "<i4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("vx1", "<f4"),
                     ("vy1", "<f4"), ("vx2", "<f4"), ("vy2", "<f4"), ("hits", "<i4"), ("missed", "<i4"), ("age", "<i4"),
                     ("det_class", "<i4"), ("wsum", "<f4"), ("has_vote", "<i4")]

# numpy view of lp_det records
DET_DTYPE = [("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("det_conf", "<f4"), ("det_class", "<i4"),
             ("cls_class", "<i4"), ("cls_conf", "<f4")]

LP_TOPK_MAX = 8


class LpTopk(C.Structure):
    """lp_topk, 64 bytes, parallel to lp_det: the k most probable classes of a detection; unused entries cls = -1, prob = 0"""
    _fields_ = [("cls", C.c_int32 * LP_TOPK_MAX), ("prob", C.c_float * LP_TOPK_MAX)]


# numpy view of lp_topk records
TOPK_DTYPE = [("cls", "<i4", (LP_TOPK_MAX,)), ("prob", "<f4", (LP_TOPK_MAX,))]

LP_QUALITY_VALID = 1
LP_RANK_CONFIG, LP_RANK_SHARPNESS = 0, 1


class LpQuality(C.Structure):
    """lp_quality, 32 bytes, parallel to lp_det: sharpness (variance of the Laplacian of the crop's luma) and exposure of a
    detection's classifier crop; the empty record is sharpness = -1, everything else 0"""
    _fields_ = [("sharpness", C.c_float), ("luma_mean", C.c_float), ("luma_var", C.c_float), ("clip_lo", C.c_float), ("clip_hi", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


# numpy view of lp_quality records
QUALITY_DTYPE = [("sharpness", "<f4"), ("luma_mean", "<f4"), ("luma_var", "<f4"), ("clip_lo", "<f4"), ("clip_hi", "<f4"), ("flags", "<i4"),
                 ("reserved", "<i4", (2,))]

LP_EVAL_MAX_GT, LP_EVAL_MAX_THR = 256, 16


class LpGt(C.Structure):
    """lp_gt, 32 bytes: one ground-truth box, parse_yolo_label's tuple"""
    _fields_ = [("cls", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("x2", C.c_int32), ("y2", C.c_int32), ("reserved", C.c_int32 * 3)]


class LpMatch(C.Structure):
    """lp_match_rec, 16 bytes, parallel to lp_det: bit j of correct = correct at threshold j; gt = the best ground truth or -1"""
    _fields_ = [("correct", C.c_uint32), ("gt", C.c_int32), ("iou", C.c_double)]


class LpEvalRow(C.Structure):
    """lp_eval_row, 16 bytes: one record in the evaluator's log"""
    _fields_ = [("conf", C.c_float), ("cls", C.c_int32), ("correct", C.c_uint32), ("frame", C.c_int32)]


class LpEvalConfig(C.Structure):
    _fields_ = [("max_gt", C.c_int), ("max_rows", C.c_int), ("n_thr", C.c_int), ("reserved0", C.c_int), ("thr", C.c_double * LP_EVAL_MAX_THR),
                ("reserved", C.c_int * 8)]


# numpy views of lp_gt, lp_match_rec and lp_eval_row records
GT_DTYPE = [("cls", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("reserved", "<i4", (3,))]
MATCH_DTYPE = [("correct", "<u4"), ("gt", "<i4"), ("iou", "<f8")]
EVAL_ROW_DTYPE = [("conf", "<f4"), ("cls", "<i4"), ("correct", "<u4"), ("frame", "<i4")]

SYMBOLS = [
    "lp_last_error", "lp_version", "lp_default_config", "lp_create", "lp_destroy", "lp_load_detector_ncnn",
    "lp_load_classifier_tensors", "lp_detect_raw", "lp_detect", "lp_run_batch", "lp_run_batch_device", "lp_classify",
    "lp_set_stream", "lp_synchronize", "lp_profile_next", "lp_profile_read", "lp_detector_info", "lp_debug_blob",
    "lp_test_conv", "lp_test_postprocess", "lp_test_nms_boxes", "lp_test_roi_resize", "lp_test_letterbox", "lp_roi_overflow",
    "lp_comm_unique_id", "lp_comm_init", "lp_gather", "lp_comm_destroy",
    "lp_tile_grid", "lp_run_tiled", "lp_run_tiled_device", "lp_test_nms_views", "lp_test_tile_views",
    "lp_view_grid", "lp_view_geometry", "lp_run_views", "lp_run_views_device", "lp_test_view_windows",
    "lp_frame_layout", "lp_set_input_format", "lp_test_convert_frames",
    "lp_track_default_config", "lp_track_config_check", "lp_tracker_create", "lp_tracker_destroy", "lp_tracker_reset",
    "lp_track_device", "lp_track", "lp_tracker_snapshot",
    "lp_inventory_default_config", "lp_inventory_config_check", "lp_inventory_create", "lp_inventory_destroy", "lp_inventory_device",
    "lp_inventory", "lp_inventory_flush", "lp_inventory_drain", "lp_inventory_open", "lp_test_set_rois", "lp_debug_rois",
    "lp_evidence_default_config", "lp_evidence_config_check", "lp_evidence_window", "lp_evidence_create", "lp_evidence_destroy",
    "lp_inventory_drain_evidence", "lp_evidence_open", "lp_test_set_frames",
    "lp_focus_default_config", "lp_focus_config_check", "lp_focus_create", "lp_focus_destroy", "lp_focus_plan", "lp_focus_state",
    "lp_run_focus_device", "lp_run_focus",
    "lp_letterbox_geometry", "lp_test_letterbox_kernel", "lp_test_roi_resize_rects",
    "lp_load_detector_onnx", "lp_load_detector_onnx_memory", "lp_detector_graph_describe",
    "lp_view_merge_default", "lp_view_merge_check", "lp_set_view_merge",
    "lp_surfaces_check", "lp_run_surfaces_device", "lp_run_views_surfaces_device", "lp_test_convert_surfaces", "lp_graph_stats",
    "lp_topk_enable", "lp_topk_buffer", "lp_topk_read", "lp_topk_select", "lp_track_topk_device", "lp_track_topk", "lp_test_topk",
    "lp_quality_enable", "lp_quality_buffer", "lp_quality_read", "lp_quality_measure", "lp_inventory_set_rank", "lp_test_quality",
    "lp_map_fixed", "lp_map_render", "lp_map_box", "lp_map_add", "lp_map_clear", "lp_run_mapped", "lp_run_mapped_device",
    "lp_test_map_views", "lp_test_map_boxes",
    "lp_eval_default_config", "lp_eval_config_check", "lp_eval_create", "lp_eval_destroy", "lp_eval_reset", "lp_eval_device", "lp_eval",
    "lp_eval_drain", "lp_eval_match",
]
LP_MAP_MAX = 64
ABI_VERSION = 310   # include/litepi.h LP_ABI_VERSION: a library built from another header is refused (load_library)

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the library and declare prototypes.  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `python yolo-litepi_amd/build.py` "
                          "(hipcc --offload-arch=gfx950); litepi has no CPU fallback")
    lib = C.CDLL(p)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    u8pp = C.POINTER(C.c_void_p)
    lib.lp_last_error.restype = C.c_char_p
    lib.lp_version.restype = C.c_int
    lib.lp_default_config.argtypes = [C.POINTER(LpConfig)]
    lib.lp_default_config.restype = None
    lib.lp_create.argtypes = [C.POINTER(LpConfig), C.POINTER(vp)]
    lib.lp_destroy.argtypes = [vp]
    lib.lp_destroy.restype = None
    lib.lp_load_detector_ncnn.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.lp_load_detector_onnx.argtypes = [vp, C.c_char_p]
    lib.lp_load_detector_onnx_memory.argtypes = [vp, vp, C.c_size_t, C.c_char_p]
    lib.lp_detector_graph_describe.argtypes = [C.c_char_p, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.lp_load_classifier_tensors.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(vp), ip]
    lib.lp_detect_raw.argtypes = [vp, vp, C.c_int, vp]
    lib.lp_detect.argtypes = [vp, u8pp, ip, ip, C.c_int, C.c_float, C.c_float, vp, ip]
    lib.lp_run_batch.argtypes = [vp, u8pp, ip, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, ip, ip, fp, C.POINTER(LpTiming)]
    lib.lp_run_batch_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_classify.argtypes = [vp, u8pp, ip, ip, C.c_int, ip, fp]
    lib.lp_set_stream.argtypes = [vp, vp]
    lib.lp_synchronize.argtypes = [vp]
    lib.lp_profile_next.argtypes = [vp, C.c_int]
    lib.lp_profile_read.argtypes = [vp, C.POINTER(LpKernelTime), C.c_int, ip]
    lib.lp_detector_info.argtypes = [vp, ip, ip, ip, C.POINTER(C.c_double)]
    lib.lp_debug_blob.argtypes = [vp, C.c_char_p, fp, C.c_int64, ip, ip, ip]
    lib.lp_test_conv.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int,
                                 C.c_int, fp, fp]
    lib.lp_test_postprocess.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_int, C.c_int, vp, ip, ip, ip]
    lib.lp_test_nms_boxes.argtypes = [vp, fp, fp, ip, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp, ip, ip, ip]
    lib.lp_test_roi_resize.argtypes = [vp, u8pp, ip, ip, C.c_int, vp]
    lib.lp_test_roi_resize_rects.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, vp]
    lib.lp_test_letterbox.argtypes = [vp, vp, C.c_int, C.c_int, vp, fp, fp, fp]
    lib.lp_test_letterbox_kernel.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, fp, fp, fp]
    lib.lp_roi_overflow.argtypes = [vp, ip, ip]
    lib.lp_comm_unique_id.argtypes = [vp]
    lib.lp_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.lp_gather.argtypes = [vp, vp, C.c_size_t, vp, C.c_int]
    lib.lp_comm_destroy.argtypes = [vp]
    tp = C.POINTER(LpTiling)
    lib.lp_tile_grid.argtypes = [C.c_int, tp, C.c_int, C.c_int, ip, ip, C.c_int]
    lib.lp_run_tiled.argtypes = [vp, u8pp, ip, ip, C.c_int, tp, C.c_float, C.c_float, C.c_int, vp, ip, ip, fp, C.POINTER(LpTiming)]
    lib.lp_run_tiled_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, tp, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_test_nms_views.argtypes = [vp, fp, fp, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp,
                                      ip, ip, ip]
    lib.lp_test_tile_views.argtypes = [vp, vp, C.c_int, C.c_int, tp, C.c_int, vp, C.c_int, ip]
    lib.lp_view_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int]
    lib.lp_view_geometry.argtypes = [C.c_int, C.c_int, C.c_int, ip, fp, fp, fp, ip, ip, ip, ip]
    lib.lp_letterbox_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp, ip, ip, ip, ip]
    lib.lp_run_views.argtypes = [vp, u8pp, ip, ip, C.c_int, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, ip, ip, fp, C.POINTER(LpTiming)]
    lib.lp_run_views_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_test_view_windows.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, vp, C.c_int]
    ffp, i64p = C.POINTER(LpFrameFormat), C.POINTER(C.c_int64)
    lib.lp_frame_layout.argtypes = [ffp, C.c_int, C.c_int, i64p, i64p]
    lib.lp_set_input_format.argtypes = [vp, ffp]
    lib.lp_test_convert_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ffp, C.c_int, vp]
    tcp = C.POINTER(LpTrackConfig)
    lib.lp_track_default_config.argtypes = [tcp]
    lib.lp_track_default_config.restype = None
    lib.lp_track_config_check.argtypes = [tcp]
    lib.lp_tracker_create.argtypes = [vp, tcp]
    lib.lp_tracker_destroy.argtypes = [vp]
    lib.lp_tracker_reset.argtypes = [vp, C.c_int]
    lib.lp_track_device.argtypes = [vp, vp, vp, C.c_int, ip, vp]
    lib.lp_track.argtypes = [vp, vp, ip, C.c_int, ip, vp]
    lib.lp_tracker_snapshot.argtypes = [vp, C.c_int, vp, C.c_int, ip, vp, ip, ip]
    icp = C.POINTER(LpInventoryConfig)
    lib.lp_inventory_default_config.argtypes = [icp]
    lib.lp_inventory_default_config.restype = None
    lib.lp_inventory_config_check.argtypes = [icp]
    lib.lp_inventory_create.argtypes = [vp, icp]
    lib.lp_inventory_destroy.argtypes = [vp]
    lib.lp_inventory_device.argtypes = [vp, vp, vp, vp, C.c_int, ip, C.c_int]
    lib.lp_inventory.argtypes = [vp, vp, ip, vp, C.c_int, ip, C.c_int]
    lib.lp_inventory_flush.argtypes = [vp, C.c_int]
    lib.lp_inventory_drain.argtypes = [vp, vp, vp, C.c_int, ip, ip]
    lib.lp_inventory_open.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    lib.lp_test_set_rois.argtypes = [vp, vp, ip, ip, C.c_int]
    lib.lp_debug_rois.argtypes = [vp, vp, ip, ip, C.c_int, ip]
    ecp = C.POINTER(LpEvidenceConfig)
    lib.lp_evidence_default_config.argtypes = [ecp]
    lib.lp_evidence_default_config.restype = None
    lib.lp_evidence_config_check.argtypes = [ecp]
    lib.lp_evidence_window.argtypes = [ecp, C.c_int, C.c_int, fp, ip, ip]
    lib.lp_evidence_create.argtypes = [vp, ecp]
    lib.lp_evidence_destroy.argtypes = [vp]
    lib.lp_inventory_drain_evidence.argtypes = [vp, vp, vp, vp, vp, C.c_int, ip, ip]
    lib.lp_evidence_open.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip]
    lib.lp_test_set_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    fcp = C.POINTER(LpFocusConfig)
    lib.lp_focus_default_config.argtypes = [fcp]
    lib.lp_focus_default_config.restype = None
    lib.lp_focus_config_check.argtypes = [fcp, C.c_int]
    lib.lp_focus_create.argtypes = [vp, fcp]
    lib.lp_focus_destroy.argtypes = [vp]
    lib.lp_focus_plan.argtypes = [vp, C.c_int, ip, ip, ip, ip, C.c_int]
    lib.lp_focus_state.argtypes = [vp, C.c_int, ip, ip]
    lib.lp_run_focus_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.c_float, C.c_float, C.c_int, vp, vp, vp]
    lib.lp_run_focus.argtypes = [vp, u8pp, ip, ip, C.c_int, ip, C.c_float, C.c_float, C.c_int, vp, ip, ip, fp, C.POINTER(LpTiming), ip]
    vmp = C.POINTER(LpViewMerge)
    lib.lp_view_merge_default.argtypes = [vmp]
    lib.lp_view_merge_default.restype = None
    lib.lp_view_merge_check.argtypes = [vmp]
    lib.lp_set_view_merge.argtypes = [vp, vmp]
    sfp, sp = C.POINTER(LpSurfaceFormat), C.POINTER(LpSurface)
    lib.lp_surfaces_check.argtypes = [sfp, sp, C.c_int]
    lib.lp_run_surfaces_device.argtypes = [vp, sfp, sp, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_run_views_surfaces_device.argtypes = [vp, sfp, sp, C.c_int, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_test_convert_surfaces.argtypes = [vp, sfp, sp, C.c_int, vp]
    lib.lp_graph_stats.argtypes = [vp, ip, i64p, i64p, i64p]
    lib.lp_topk_enable.argtypes = [vp, C.c_int]
    lib.lp_topk_buffer.argtypes = [vp, C.POINTER(vp), ip]
    lib.lp_topk_read.argtypes = [vp, vp, C.c_int]
    lib.lp_topk_select.argtypes = [fp, C.c_int, C.c_int, C.POINTER(LpTopk)]
    lib.lp_track_topk_device.argtypes = [vp, vp, vp, vp, C.c_int, ip, vp]
    lib.lp_track_topk.argtypes = [vp, vp, ip, vp, C.c_int, ip, vp]
    lib.lp_test_topk.argtypes = [vp, fp, C.c_int, ip, ip, C.c_int, vp]
    lib.lp_quality_enable.argtypes = [vp, C.c_int]
    lib.lp_quality_buffer.argtypes = [vp, C.POINTER(vp)]
    lib.lp_quality_read.argtypes = [vp, vp, C.c_int]
    lib.lp_quality_measure.argtypes = [vp, C.c_int, C.POINTER(LpQuality)]
    lib.lp_inventory_set_rank.argtypes = [vp, C.c_int]
    lib.lp_test_quality.argtypes = [vp, C.c_int, vp]
    lib.lp_map_fixed.argtypes = [fp, C.c_int, C.c_int, C.c_int, vp]
    lib.lp_map_render.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp]
    lib.lp_map_box.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, fp]
    lib.lp_map_add.argtypes = [vp, fp, C.c_int, C.c_int, ip]
    lib.lp_map_clear.argtypes = [vp]
    lib.lp_run_mapped.argtypes = [vp, u8pp, ip, ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, ip, ip, fp,
                                  C.POINTER(LpTiming)]
    lib.lp_run_mapped_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    lib.lp_test_map_views.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, vp, C.c_int]
    lib.lp_test_map_boxes.argtypes = [vp, C.c_int, fp, C.c_int, fp]
    evp = C.POINTER(LpEvalConfig)
    lib.lp_eval_default_config.argtypes = [evp]
    lib.lp_eval_default_config.restype = None
    lib.lp_eval_config_check.argtypes = [evp]
    lib.lp_eval_create.argtypes = [vp, evp]
    lib.lp_eval_destroy.argtypes = [vp]
    lib.lp_eval_reset.argtypes = [vp]
    lib.lp_eval_device.argtypes = [vp, vp, vp, C.c_int, vp, ip, vp]
    lib.lp_eval.argtypes = [vp, vp, ip, C.c_int, vp, ip, vp]
    lib.lp_eval_drain.argtypes = [vp, vp, C.c_int, ip, ip, ip, ip]
    lib.lp_eval_match.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp]
    for s in SYMBOLS:
        if s not in ("lp_eval_default_config", "lp_last_error", "lp_default_config", "lp_destroy", "lp_track_default_config", "lp_inventory_default_config",
                     "lp_evidence_default_config", "lp_focus_default_config", "lp_view_merge_default"):
            getattr(lib, s).restype = C.c_int
    got = lib.lp_version()
    if got != ABI_VERSION:
        raise ImportError(f"{p} has ABI version {got}, these bindings need {ABI_VERSION}: rebuild with `python yolo-litepi_amd/build.py`")
    if path is None:
        _lib = lib
    return lib


class LitepiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"litepi error {code}: {msg}")
        self.code = code


def check(lib: C.CDLL, rc: int) -> None:
    if rc != 0:
        raise LitepiError(rc, lib.lp_last_error().decode(errors="replace"))
