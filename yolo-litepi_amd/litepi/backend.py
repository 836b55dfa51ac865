"""Drop-in replacements for the three classes the reference's ``main()`` builds from its CLI
flags (``src/tt100k/pipeline/e2e.py``): ``NCNNDetector`` (:195), ``PyTorchClassifier`` (:350)
and ``HybridPipeline`` (:399), plus the ``PipelineMetrics`` dataclass (:34).  Same constructor
arguments, same method signatures, same return types and empty-result quirks; the arithmetic
runs in liblitepi_hip.so on an MI355X instead of NCNN / torch-CPU / NumPy.

``Engine`` is the thin object wrapper over the C-ABI handle that the three classes share.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import (DET_DTYPE, QUALITY_DTYPE, SIGN_DTYPE, TOPK_DTYPE, TRACK_DTYPE, TRACK_STATE_DTYPE, LpConfig, LpFrameFormat, LpInventoryConfig, LpKernelTime, LpTiming,
                   LpTiling, LpTrackConfig, check)
from .pixfmt import CSC_MATRICES, PIXEL_FORMATS, nv12_frame_hw
from .surfaces import Surface, surface_array, surface_format, surface_from_tensors, surfaces_check  # noqa: F401  (re-exported)

_PREC = {"fp32": _ffi.LP_FP32, "fp16": _ffi.LP_FP16, "float32": _ffi.LP_FP32, "float16": _ffi.LP_FP16, "half": _ffi.LP_FP16}


def _as_bgr(img: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected a BGR uint8 HxWx3 image, got shape {img.shape}")
    return a


def _as_nv12(img: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.uint8)
    nv12_frame_hw(a.shape)   # ValueError for anything but (H * 3 // 2, W)
    return a


def _frame_format(pixfmt: str = "bgr", matrix: str = "bt601", pitch: int = 0, uv_offset: int = 0, frame_stride: int = 0) -> LpFrameFormat:
    if pixfmt not in PIXEL_FORMATS:
        raise ValueError(f"unknown pixel format {pixfmt!r} (one of {sorted(PIXEL_FORMATS)})")
    if matrix not in CSC_MATRICES:
        raise ValueError(f"unknown colour matrix {matrix!r} (one of {sorted(CSC_MATRICES)})")
    f = LpFrameFormat()
    f.pixfmt, f.matrix, f.pitch, f.uv_offset, f.frame_stride = PIXEL_FORMATS[pixfmt], CSC_MATRICES[matrix], int(pitch), int(uv_offset), int(frame_stride)
    return f


def frame_layout(H: int, W: int, pixfmt: str = "nv12", matrix: str = "bt601", pitch: int = 0, uv_offset: int = 0,
                 frame_stride: int = 0) -> Tuple[int, int]:
    """(uv_offset, frame_bytes) of an H x W frame in the given format with the zeros resolved (lp_frame_layout: host only, no
    GPU needed); LitepiError(LP_ERR_ARG) for a layout the size rules out."""
    lib = _ffi.load_library()
    f = _frame_format(pixfmt, matrix, pitch, uv_offset, frame_stride)
    uv, nb = C.c_int64(), C.c_int64()
    check(lib, lib.lp_frame_layout(C.byref(f), int(H), int(W), C.byref(uv), C.byref(nb)))
    return uv.value, nb.value


CLS_ARCHS = ("resnet18", "efficientnet", "mobilenetv2", "shufflenetv2")   # the --clf_arch choices of e2e.py:1021


def _tiling(overlap: int, full_frame: bool) -> LpTiling:
    t = LpTiling()
    t.overlap, t.full_frame = int(overlap), int(bool(full_frame))
    return t


def tile_grid(det_input: int, H: int, W: int, overlap: int = 128, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
    """The views of an H x W frame in tiled mode (lp_tile_grid: host only, no GPU needed): (x, y, w, h) source windows,
    (x0, y0, S, S) for a crop and (-1, -1, W, H) for the letterboxed whole frame, in the library's view order."""
    lib = _ffi.load_library()
    t = _tiling(overlap, full_frame)
    n = C.c_int()
    check(lib, lib.lp_tile_grid(int(det_input), C.byref(t), int(H), int(W), C.byref(n), None, 0))
    buf = (C.c_int * (4 * n.value))()
    check(lib, lib.lp_tile_grid(int(det_input), C.byref(t), int(H), int(W), C.byref(n), buf, n.value))
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def _view_array(views) -> np.ndarray:
    """a view list as the [n, 4] int32 array the library takes: (x, y, w, h) windows, "full" (or any x = -1) = the whole frame"""
    rows = [(-1, -1, 0, 0) if isinstance(v, str) and v == "full" else tuple(int(c) for c in v) for v in views]
    if any(len(r) != 4 for r in rows):
        raise ValueError('a view is (x, y, w, h) or "full"')
    return np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 4))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _id_array(ids) -> np.ndarray:
    """a list of map ids as the int32 array the library takes"""
    return np.ascontiguousarray(np.asarray(list(ids) if ids is not None else [], dtype=np.int32).reshape(-1))


def view_grid(tile: int, H: int, W: int, overlap: int = 0, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
    """The window grid of an H x W frame (lp_view_grid: host only, no GPU needed): (x, y, w, h) windows of side `tile` (or the
    frame's, where it is shorter) overlapping by `overlap`, row-major, behind (-1, -1, W, H) for the whole frame."""
    lib = _ffi.load_library()
    n = C.c_int()
    check(lib, lib.lp_view_grid(int(tile), int(overlap), int(bool(full_frame)), int(H), int(W), C.byref(n), None, 0))
    buf = (C.c_int * (4 * n.value))()
    check(lib, lib.lp_view_grid(int(tile), int(overlap), int(bool(full_frame)), int(H), int(W), C.byref(n), buf, n.value))
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n.value)]


def view_geometry(det_input: int, H: int, W: int, view) -> Dict[str, object]:
    """The geometry of one view of an H x W frame (lp_view_geometry: host only): ratio, pad_w, pad_h (float32 values), new_w,
    new_h, top, left."""
    lib = _ffi.load_library()
    v = _view_array([view])
    r, pw, ph = C.c_float(), C.c_float(), C.c_float()
    nw, nh, top, left = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib, lib.lp_view_geometry(int(det_input), int(H), int(W), _ip(v), C.byref(r), C.byref(pw), C.byref(ph), C.byref(nw), C.byref(nh),
                                    C.byref(top), C.byref(left)))
    return dict(ratio=np.float32(r.value), pad_w=np.float32(pw.value), pad_h=np.float32(ph.value), new_w=nw.value, new_h=nh.value,
                top=top.value, left=left.value)


def letterbox_geometry(det_h: int, det_w: int, H: int, W: int) -> Dict[str, object]:
    """The letterbox of an H x W image into a det_h x det_w detector input (lp_letterbox_geometry: host only), the reference's
    letterbox(img, (det_h, det_w)): ratio, pad_w, pad_h (float32 values), new_w, new_h, top, left."""
    lib = _ffi.load_library()
    r, pw, ph = C.c_float(), C.c_float(), C.c_float()
    nw, nh, top, left = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib, lib.lp_letterbox_geometry(int(det_h), int(det_w), int(H), int(W), C.byref(r), C.byref(pw), C.byref(ph), C.byref(nw),
                                         C.byref(nh), C.byref(top), C.byref(left)))
    return dict(ratio=np.float32(r.value), pad_w=np.float32(pw.value), pad_h=np.float32(ph.value), new_w=nw.value, new_h=nh.value,
                top=top.value, left=left.value)


def _map_table(a, what: str = "xy") -> np.ndarray:
    """a map table as the contiguous [S, S, 2] array the library takes"""
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 2:
        raise ValueError(f"{what} is [S, S, 2] (got {a.shape})")
    return a


def map_fixed(xy, H: int, W: int) -> np.ndarray:
    """The fixed-point table of a map xy [S, S, 2] float32 (frame positions (x, y) of the view's pixels, pixel centres at
    integers) for H x W frames (lp_map_fixed: host only): [S, S, 2] int32 with 5 fractional bits."""
    lib = _ffi.load_library()
    xy = np.ascontiguousarray(_map_table(xy), dtype=np.float32)
    out = np.zeros(xy.shape, dtype=np.int32)
    check(lib, lib.lp_map_fixed(xy.ctypes.data_as(C.POINTER(C.c_float)), xy.shape[0], int(H), int(W), out.ctypes.data))
    return out


def map_render(fixed, frame: np.ndarray) -> np.ndarray:
    """The view [S, S, 3] of a BGR frame through a fixed table (lp_map_render: host only)."""
    lib = _ffi.load_library()
    fixed = np.ascontiguousarray(_map_table(fixed, "fixed"), dtype=np.int32)
    frame = _as_bgr(frame)
    S = fixed.shape[0]
    out = np.zeros((S, S, 3), dtype=np.uint8)
    check(lib, lib.lp_map_render(fixed.ctypes.data, S, frame.ctypes.data, frame.shape[0], frame.shape[1], out.ctypes.data))
    return out


def map_box(fixed, H: int, W: int, boxes) -> np.ndarray:
    """View boxes [n, 4] (x1, y1, x2, y2) as frame boxes through a fixed table (lp_map_box: host only), float32."""
    lib = _ffi.load_library()
    fixed = np.ascontiguousarray(_map_table(fixed, "fixed"), dtype=np.int32)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
    out = np.zeros_like(b)
    fp = C.POINTER(C.c_float)
    for k in range(len(b)):
        check(lib, lib.lp_map_box(fixed.ctypes.data, fixed.shape[0], int(H), int(W), b[k].ctypes.data_as(fp), out[k].ctypes.data_as(fp)))
    return out


TRACK_CONFIG_FIELDS = ("n_streams", "max_tracks", "iou_match", "max_age", "min_hits", "new_conf", "vote_decay", "class_gate", "motion")


def track_config(**cfg) -> LpTrackConfig:
    """lp_track_config with the library's defaults (lp_track_default_config) and the given fields (host only, no GPU needed)."""
    lib = _ffi.load_library()
    c = LpTrackConfig()
    lib.lp_track_default_config(C.byref(c))
    for k, v in cfg.items():
        if k not in TRACK_CONFIG_FIELDS:
            raise TypeError(f"unknown tracker setting {k!r} (one of {TRACK_CONFIG_FIELDS})")
        setattr(c, k, v)
    return c


def track_config_check(cfg: Optional[LpTrackConfig]) -> int:
    """lp_track_config_check's status for a configuration (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_track_config_check(C.byref(cfg) if cfg is not None else None)


def topk_select(p, k: int) -> np.ndarray:
    """lp_topk_select (host only, no GPU needed): the top-k selection rule on one distribution p [nc] -> one TOPK_DTYPE
    record; LitepiError(LP_ERR_ARG) for an empty p or k outside 1..8."""
    lib = _ffi.load_library()
    a = np.ascontiguousarray(p, dtype=np.float32).reshape(-1)
    out = np.zeros(1, dtype=TOPK_DTYPE)
    check(lib, lib.lp_topk_select(a.ctypes.data_as(C.POINTER(C.c_float)), len(a), int(k), C.cast(out.ctypes.data, C.POINTER(_ffi.LpTopk))))
    return out[0]


TRACK_VOTES = ("top1", "distribution")


def check_topk_options(topk, track_vote: str, track: bool) -> int:
    """the rules HybridPipeline and the CLI share for topk / track_vote; returns k (0 = off).  ValueError names both options."""
    k = 0 if topk is None else int(topk)
    if not 0 <= k <= _ffi.LP_TOPK_MAX:
        raise ValueError(f"topk = {topk!r} outside 0..{_ffi.LP_TOPK_MAX}")
    if track_vote not in TRACK_VOTES:
        raise ValueError(f"track_vote = {track_vote!r} is not one of {TRACK_VOTES}")
    if track_vote == "distribution" and not (track and k >= 1):
        raise ValueError("track_vote='distribution' needs track=True and topk >= 1 (--track_vote distribution needs --track and --topk K)")
    return k


def quality_measure(crop) -> np.ndarray:
    """lp_quality_measure (host only, no GPU needed): the crop quality rule on one [S, S, 3] uint8 RGB crop -> one QUALITY_DTYPE
    record; LitepiError(LP_ERR_ARG) for S outside 3..1024.  ValueError for a crop that is not square with 3 channels."""
    lib = _ffi.load_library()
    a = np.ascontiguousarray(crop, dtype=np.uint8)
    if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
        raise ValueError(f"a crop is [S, S, 3] uint8 RGB, got shape {a.shape}")
    out = np.zeros(1, dtype=QUALITY_DTYPE)
    check(lib, lib.lp_quality_measure(a.ctypes.data, a.shape[0], C.cast(out.ctypes.data, C.POINTER(_ffi.LpQuality))))
    return out[0]


EVAL_CONFIG_FIELDS = ("max_gt", "max_rows", "thr")


def eval_config(**cfg) -> _ffi.LpEvalConfig:
    """lp_eval_config with the library's defaults (lp_eval_default_config) and the given fields: max_gt, max_rows, and thr, a
    sequence of 1..16 IoU thresholds (n_thr is its length).  Host only, no GPU needed."""
    lib = _ffi.load_library()
    c = _ffi.LpEvalConfig()
    lib.lp_eval_default_config(C.byref(c))
    for k, v in cfg.items():
        if k not in EVAL_CONFIG_FIELDS:
            raise TypeError(f"unknown evaluator setting {k!r} (one of {EVAL_CONFIG_FIELDS})")
        if k == "thr":
            t = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if not 1 <= len(t) <= _ffi.LP_EVAL_MAX_THR:
                raise ValueError(f"thr holds 1..{_ffi.LP_EVAL_MAX_THR} thresholds (got {len(t)})")
            c.n_thr = len(t)
            for j in range(_ffi.LP_EVAL_MAX_THR):
                c.thr[j] = float(t[j]) if j < len(t) else 0.0
        else:
            setattr(c, k, int(v))
    return c


def eval_config_check(cfg: Optional[_ffi.LpEvalConfig]) -> int:
    """lp_eval_config_check's status for a configuration (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_eval_config_check(C.byref(cfg) if cfg is not None else None)


def gt_records(gts) -> np.ndarray:
    """one frame's ground truth, [(cls, x1, y1, x2, y2), ...] (parse_yolo_label's tuples) or GT_DTYPE records -> GT_DTYPE records"""
    if isinstance(gts, np.ndarray) and gts.dtype.names:
        return np.ascontiguousarray(gts, dtype=_ffi.GT_DTYPE).reshape(-1)
    a = np.asarray(gts, dtype=np.int64).reshape(-1, 5)
    if len(a) and (np.abs(a) > 2 ** 31 - 1).any():
        raise ValueError("a ground-truth value does not fit int32")
    out = np.zeros(len(a), dtype=_ffi.GT_DTYPE)
    for k, name in enumerate(("cls", "x1", "y1", "x2", "y2")):
        out[name] = a[:, k]
    return out


def eval_match(dets, gts, thr=None) -> np.ndarray:
    """lp_eval_match (host only, no GPU needed): the evaluator's matching rule on one frame.  dets: DET_DTYPE records, gts: as
    gt_records takes them, thr: the IoU thresholds (None: np.arange(0.5, 1.0, 0.05)) -> one MATCH_DTYPE record per detection."""
    lib = _ffi.load_library()
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1)
    g = gt_records(gts)
    t = np.ascontiguousarray(np.arange(0.5, 1.0, 0.05) if thr is None else thr, dtype=np.float64).reshape(-1)
    out = np.zeros(len(d), dtype=_ffi.MATCH_DTYPE)
    check(lib, lib.lp_eval_match(d.ctypes.data, len(d), g.ctypes.data, len(g), t.ctypes.data_as(C.POINTER(C.c_double)), len(t), out.ctypes.data))
    return out


def check_eval_options(evaluate, gts, n_images: Optional[int] = None) -> None:
    """the rule HybridPipeline.run_batch applies to evaluate / gts: one needs the other, and gts holds one list per image"""
    if evaluate and gts is None:
        raise ValueError("a pipeline constructed with evaluate needs run_batch(gts=...): one list of (cls, x1, y1, x2, y2) per image")
    if gts is not None and not evaluate:
        raise ValueError("run_batch(gts=...) needs a pipeline constructed with evaluate=True or an evaluator configuration")
    if gts is not None and n_images is not None and len(gts) != n_images:
        raise ValueError(f"gts must hold one list per image ({n_images}), got {len(gts)}")


INVENTORY_RANKS = {"config": _ffi.LP_RANK_CONFIG, "sharpness": _ffi.LP_RANK_SHARPNESS}
QUALITY_RESULT_KEYS = ("sharpness", "luma_mean", "clip_lo", "clip_hi")


def check_quality_options(quality, inventory):
    """the rules HybridPipeline shares with the CLI for quality / inventory best="sharpness": returns (quality on, rank name,
    the inventory settings without the rank).  "sharpness" is no lp_best: the settings keep the default `best`, the rank is set
    on the created inventory (Engine.inventory_set_rank) and quality is switched on."""
    inv = dict(inventory) if isinstance(inventory, dict) else {}
    rank = "config"
    if inv.get("best") == "sharpness":
        del inv["best"]
        rank = "sharpness"
        if not int(inv.get("keep_crops", 1)):
            raise ValueError("inventory best='sharpness' needs keep_crops: the sharpness is measured on the crops the inventory keeps")
    return bool(quality) or rank == "sharpness", rank, inv


INVENTORY_CONFIG_FIELDS = ("max_signs", "keep_crops", "best", "min_hits")
INVENTORY_BEST = {"area": _ffi.LP_BEST_AREA, "det_conf": _ffi.LP_BEST_DET_CONF, "cls_conf": _ffi.LP_BEST_CLS_CONF}


def inventory_config(**cfg) -> LpInventoryConfig:
    """lp_inventory_config with the library's defaults and the given fields (host only, no GPU needed); best may be a name of
    INVENTORY_BEST."""
    lib = _ffi.load_library()
    c = LpInventoryConfig()
    lib.lp_inventory_default_config(C.byref(c))
    for k, v in cfg.items():
        if k not in INVENTORY_CONFIG_FIELDS:
            raise TypeError(f"unknown inventory setting {k!r} (one of {INVENTORY_CONFIG_FIELDS})")
        if k == "best" and isinstance(v, str):
            if v not in INVENTORY_BEST:
                raise ValueError(f"best must be one of {tuple(INVENTORY_BEST)}, got {v!r}")
            v = INVENTORY_BEST[v]
        setattr(c, k, int(v))
    return c


def inventory_config_check(cfg: Optional[LpInventoryConfig]) -> int:
    """lp_inventory_config_check's status for a configuration (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_inventory_config_check(C.byref(cfg) if cfg is not None else None)


EVIDENCE_CONFIG_FIELDS = ("size", "scale")


def evidence_config(**cfg) -> _ffi.LpEvidenceConfig:
    """lp_evidence_config with the library's defaults and the given fields (host only, no GPU needed)."""
    lib = _ffi.load_library()
    c = _ffi.LpEvidenceConfig()
    lib.lp_evidence_default_config(C.byref(c))
    for k, v in cfg.items():
        if k not in EVIDENCE_CONFIG_FIELDS:
            raise TypeError(f"unknown evidence setting {k!r} (one of {EVIDENCE_CONFIG_FIELDS})")
        setattr(c, k, float(v) if k == "scale" else int(v))
    return c


def evidence_config_check(cfg: Optional[_ffi.LpEvidenceConfig]) -> int:
    """lp_evidence_config_check's status for a configuration (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_evidence_config_check(C.byref(cfg) if cfg is not None else None)


def evidence_window(cfg: _ffi.LpEvidenceConfig, H: int, W: int, box) -> Tuple[Tuple[int, int, int, int], bool]:
    """lp_evidence_window: ((x, y, w, h), has) of box (x1, y1, x2, y2) on an H x W frame (host only, no GPU needed)."""
    lib = _ffi.load_library()
    b = np.ascontiguousarray(box, dtype=np.float32).reshape(4)
    win, has = np.zeros(4, np.int32), C.c_int()
    check(lib, lib.lp_evidence_window(C.byref(cfg), int(H), int(W), b.ctypes.data_as(C.POINTER(C.c_float)), _ip(win), C.byref(has)))
    return tuple(int(v) for v in win), bool(has.value)


FOCUS_CONFIG_FIELDS = ("slots", "side_min", "side_max", "margin", "small_px", "border", "sweep", "sweep_overlap")


VIEW_MATCHES = {"iou": _ffi.LP_MATCH_IOU, "ios": _ffi.LP_MATCH_IOS}
VIEW_MERGES = {"nms": _ffi.LP_MERGE_SUPPRESS, "union": _ffi.LP_MERGE_UNION}


def view_merge_config(match: str = "iou", merge: str = "nms", threshold: float = 0.0) -> _ffi.LpViewMerge:
    """lp_view_merge from the names of its settings (host only, no GPU needed); ValueError for an unknown name."""
    if match not in VIEW_MATCHES:
        raise ValueError(f"unknown view match {match!r} (one of {sorted(VIEW_MATCHES)})")
    if merge not in VIEW_MERGES:
        raise ValueError(f"unknown view merge {merge!r} (one of {sorted(VIEW_MERGES)})")
    m = _ffi.LpViewMerge()
    m.metric, m.mode, m.threshold = VIEW_MATCHES[match], VIEW_MERGES[merge], float(threshold)
    return m


def view_merge_check(cfg: Optional[_ffi.LpViewMerge]) -> int:
    """lp_view_merge_check's status for a setting (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_view_merge_check(C.byref(cfg) if cfg is not None else None)


def focus_config(**cfg) -> _ffi.LpFocusConfig:
    """lp_focus_config with the library's defaults (lp_focus_default_config) and the given fields (host only, no GPU needed)."""
    lib = _ffi.load_library()
    c = _ffi.LpFocusConfig()
    lib.lp_focus_default_config(C.byref(c))
    for k, v in cfg.items():
        if k not in FOCUS_CONFIG_FIELDS:
            raise TypeError(f"unknown focus setting {k!r} (one of {FOCUS_CONFIG_FIELDS})")
        setattr(c, k, float(v) if k in ("margin", "small_px") else int(v))
    return c


def focus_config_check(cfg: Optional[_ffi.LpFocusConfig], det_input: int) -> int:
    """lp_focus_config_check's status for a configuration (host only, no GPU needed)."""
    lib = _ffi.load_library()
    return lib.lp_focus_config_check(C.byref(cfg) if cfg is not None else None, int(det_input))


def detector_graph_describe(model_path: str, bin_path: Optional[str] = None) -> List[str]:
    """The layers a model file lowers to, one line each without names (lp_detector_graph_describe; no device needed):
    "<type> <n_in> <n_out> <params> <crc32 of weight> <crc32 of bias>".  bin_path None: model_path is an ONNX file."""
    lib = _ffi.load_library()
    need = C.c_size_t()
    m, bn = os.fsencode(model_path), None if bin_path is None else os.fsencode(bin_path)
    check(lib, lib.lp_detector_graph_describe(m, bn, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    check(lib, lib.lp_detector_graph_describe(m, bn, buf, need.value, C.byref(need)))
    return buf.value.decode().splitlines()


def det_input_hw(size) -> Tuple[int, int]:
    """A detector input size as (rows, columns): an int is a square, a pair is the reference's letterbox shape (rows, columns)."""
    if isinstance(size, (tuple, list, np.ndarray)):
        if len(size) != 2:
            raise ValueError(f"a detector input size is an int or (rows, columns), got {size!r}")
        return int(size[0]), int(size[1])
    return int(size), int(size)


def _square_only(size, what: str) -> None:
    h, w = det_input_hw(size)
    if h != w:
        raise ValueError(f"{what} needs a square detector input; got {h}x{w} (rows x columns): frame views on a rectangular "
                         f"input are not supported")


class Engine:
    """One GPU pipeline handle (not thread-safe; one per GPU)."""

    def __init__(self, precision: str = "fp16", max_batch: int = 1, max_det: int = 300, num_classes: int = 58,
                 det_input=640, cls_input: int = 64, device: int = 0, max_rois: int = 0, conv_impl: int = 0,
                 numerics: str = "e2e", cls_arch: str = "shufflenetv2"):
        """numerics: "e2e" = HybridPipeline of e2e.py (default), "e2e_optimize" = HybridPipelineOptimized of e2e_optimize.py
        (other ROI clip rule, cv2-linear ROI resize).  cls_arch: "shufflenetv2" | "resnet18" | "mobilenetv2" | "efficientnet"
        (the four choices of build_classifier, e2e.py:320-333).  det_input: an int (square) or (rows, columns), both multiples of
        32 (lp_config::det_input_h); the frame-view calls (tiled, views, focus) need a square."""
        self.lib = _ffi.load_library()
        cfg = LpConfig()
        self.lib.lp_default_config(C.byref(cfg))
        self.det_hw = det_input_hw(det_input)
        cfg.device, cfg.precision, cfg.max_batch, cfg.max_det = device, _PREC[precision], max_batch, max_det
        cfg.num_classes, cfg.det_input, cfg.cls_input, cfg.max_rois, cfg.conv_impl = num_classes, self.det_hw[1], cls_input, max_rois, conv_impl
        cfg.det_input_h = self.det_hw[0] if isinstance(det_input, (tuple, list, np.ndarray)) else 0   # (640, 640) = 640: the same handle
        cfg.numerics = {"e2e": 0, "e2e_optimize": 1}[numerics]
        cfg.cls_arch = {"shufflenetv2": 0, "resnet18": 1, "mobilenetv2": 2, "efficientnet": 3}[cls_arch]
        self.numerics, self.cls_arch = numerics, cls_arch
        self.cfg = cfg
        self.precision = precision
        self._h = C.c_void_p()
        check(self.lib, self.lib.lp_create(C.byref(cfg), C.byref(self._h)))
        self.has_detector = False
        self.has_classifier = False
        self.pixel_format, self.csc_matrix, self._tight_frames = "bgr", "bt601", True

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.lp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- models ---------------------------------------------------------------------------
    def load_detector(self, param_path: str, bin_path: Optional[str] = None) -> None:
        """An NCNN .param / .bin pair, or one .onnx file (load_detector_onnx)."""
        if bin_path is None:
            if not str(param_path).lower().endswith(".onnx"):
                raise ValueError(f"load_detector({param_path!r}): one argument is an .onnx file; an NCNN model is a .param and a .bin")
            return self.load_detector_onnx(param_path)
        check(self.lib, self.lib.lp_load_detector_ncnn(self._h, os.fsencode(param_path), os.fsencode(bin_path)))
        self._detector_loaded()

    def load_detector_onnx(self, onnx_path) -> None:
        """An ONNX export of the detector (lp_load_detector_onnx), or the bytes of one (lp_load_detector_onnx_memory): the same
        plan and the same results as the NCNN export of that model."""
        if isinstance(onnx_path, (bytes, bytearray, memoryview)):
            data = bytes(onnx_path)
            check(self.lib, self.lib.lp_load_detector_onnx_memory(self._h, data, len(data), b"<memory>"))
        else:
            check(self.lib, self.lib.lp_load_detector_onnx(self._h, os.fsencode(onnx_path)))
        self._detector_loaded()

    def _detector_loaded(self) -> None:
        self.has_detector = True
        a, nc, rm, macs = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(self.lib, self.lib.lp_detector_info(self._h, C.byref(a), C.byref(nc), C.byref(rm), C.byref(macs)))
        self.num_anchors, self.det_classes, self.reg_max, self.det_macs = a.value, nc.value, rm.value, macs.value

    def load_classifier(self, state_dict: Dict[str, object]) -> None:
        """state_dict: torchvision shufflenet_v2_x1_0 keys -> torch tensors or ndarrays."""
        names, arrays = [], []
        for k, v in state_dict.items():
            if k.endswith("num_batches_tracked"):
                continue
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            names.append(k.encode())
            arrays.append(np.ascontiguousarray(a, dtype=np.float32))
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_data = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
        shapes = [np.asarray(a.shape, dtype=np.int64) for a in arrays]
        c_shapes = (C.c_void_p * n)(*[s.ctypes.data for s in shapes])
        c_ndims = (C.c_int * n)(*[a.ndim for a in arrays])
        check(self.lib, self.lib.lp_load_classifier_tensors(self._h, n, c_names, c_data, c_shapes, c_ndims))
        self.has_classifier = True

    # ---- inference ---------------------------------------------------------------------------
    def detect_raw(self, bgr: np.ndarray) -> np.ndarray:
        """uint8 BGR [B,SH,SW,3] -> fp32 out0 [B,4+nc,A] (parity hook for ex.extract('out0'))."""
        a = np.ascontiguousarray(bgr, dtype=np.uint8)
        SH, SW = self.det_hw
        if a.ndim == 3:
            a = a[None]
        if a.shape[1:] != (SH, SW, 3):
            raise ValueError(f"detect_raw expects [B,{SH},{SW},3], got {a.shape}")
        out = np.empty((a.shape[0], 4 + self.det_classes, self.num_anchors), np.float32)
        check(self.lib, self.lib.lp_detect_raw(self._h, a.ctypes.data, a.shape[0], out.ctypes.data))
        return out

    # ---- pixel format of the frames ------------------------------------------------------------
    def set_input_format(self, pixfmt: str = "bgr", matrix: str = "bt601", pitch: int = 0, uv_offset: int = 0,
                         frame_stride: int = 0) -> None:
        """The format of the frames given to the next detect / run_batch / run_tiled calls and their device twins
        (lp_set_input_format).  "nv12" host frames are uint8 arrays of shape (H * 3 // 2, W)."""
        f = _frame_format(pixfmt, matrix, pitch, uv_offset, frame_stride)
        check(self.lib, self.lib.lp_set_input_format(self._h, C.byref(f)))
        self.pixel_format, self.csc_matrix = pixfmt, matrix
        self._tight_frames = not (pitch or uv_offset)

    def frame_layout(self, H: int, W: int, **fmt) -> Tuple[int, int]:
        return frame_layout(H, W, **fmt)

    # ---- frame NMS of views ----------------------------------------------------------------------
    def set_view_merge(self, match: str = "iou", merge: str = "nms", threshold: float = 0.0) -> None:
        """How the frame NMS of the next run_tiled / run_views / run_focus calls, their device twins and test_nms_views merges a
        frame's views (lp_set_view_merge).  match: "iou" or "ios" (intersection over the smaller box); merge: "nms" (the keeper's
        own box) or "union" (the box around the keeper and everything it absorbs); threshold: 0 = the call's iou."""
        m = view_merge_config(match, merge, threshold)
        check(self.lib, self.lib.lp_set_view_merge(self._h, C.byref(m)))
        self.view_merge = (match, merge, float(threshold))

    def frame_hw(self, frame: np.ndarray) -> Tuple[int, int]:
        """(H, W) of a host frame in the engine's pixel format."""
        return nv12_frame_hw(frame.shape) if self.pixel_format == "nv12" else (frame.shape[0], frame.shape[1])

    def _img_args(self, images: Sequence[np.ndarray], frames: bool = False):
        """ctypes arguments of host images; frames=True: they are frames in the engine's pixel format (everything else --
        classifier crops, the test hooks -- is packed BGR)."""
        if frames and self.pixel_format == "nv12":
            if not self._tight_frames:
                raise ValueError("host NV12 arrays are tight (H * 3 // 2, W): a pitch / uv_offset describes device-resident frames")
            imgs = [_as_nv12(i) for i in images]
            sizes = [nv12_frame_hw(i.shape) for i in imgs]
        else:
            imgs = [_as_bgr(i) for i in images]
            sizes = [(i.shape[0], i.shape[1]) for i in imgs]
        n = len(imgs)
        ptrs = (C.c_void_p * n)(*[i.ctypes.data for i in imgs])
        hs = (C.c_int * n)(*[s[0] for s in sizes])
        ws = (C.c_int * n)(*[s[1] for s in sizes])
        return imgs, ptrs, hs, ws

    def detect(self, images: Sequence[np.ndarray], conf: float, iou: float):
        imgs, ptrs, hs, ws = self._img_args(images, frames=True)
        B = len(imgs)
        dets = np.zeros((B, self.cfg.max_det), dtype=DET_DTYPE)
        counts = (C.c_int * B)()
        check(self.lib, self.lib.lp_detect(self._h, ptrs, hs, ws, B, conf, iou, dets.ctypes.data, counts))
        return dets, np.array(counts[:], dtype=np.int64)

    def _run_staged(self, fn, images: Sequence[np.ndarray], extra: tuple, conf: float, iou: float, min_area: int):
        """One staged host call (lp_run_batch, lp_run_tiled, lp_run_views; `extra`: the arguments between B and conf):
        (records [B, max_det], counts, num_det, timing), and last_det_conf_avg."""
        imgs, ptrs, hs, ws = self._img_args(images, frames=True)
        B = len(imgs)
        dets = np.zeros((B, self.cfg.max_det), dtype=DET_DTYPE)
        counts, num_det = (C.c_int * B)(), (C.c_int * B)()
        conf_avg = (C.c_float * B)()
        timing = LpTiming()
        check(self.lib, fn(self._h, ptrs, hs, ws, B, *extra, conf, iou, int(min_area), dets.ctypes.data, counts, num_det, conf_avg,
                           C.byref(timing)))
        self.last_det_conf_avg = np.array(conf_avg[:], dtype=np.float32)
        return dets, np.array(counts[:], dtype=np.int64), np.array(num_det[:], dtype=np.int64), timing

    def run_batch(self, images: Sequence[np.ndarray], conf: float, iou: float, min_area: int):
        return self._run_staged(self.lib.lp_run_batch, images, (), conf, iou, min_area)

    def run_batch_device(self, dev_imgs: int, B: int, H: int, W: int, conf: float, iou: float, min_area: int,
                         dev_dets: int, dev_counts: int) -> None:
        check(self.lib, self.lib.lp_run_batch_device(self._h, C.c_void_p(dev_imgs), B, H, W, conf, iou, int(min_area),
                                                     C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    # ---- tiled inference of large frames ------------------------------------------------------
    def tile_grid(self, H: int, W: int, overlap: int = 128, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
        return tile_grid(self.cfg.det_input, H, W, overlap, full_frame)

    def run_tiled(self, images: Sequence[np.ndarray], conf: float, iou: float, min_area: int, overlap: int = 128,
                  full_frame: bool = True):
        """run_batch with every frame seen through its views (lp_run_tiled): same return values, per frame."""
        t = _tiling(overlap, full_frame)
        return self._run_staged(self.lib.lp_run_tiled, images, (C.byref(t),), conf, iou, min_area)

    def run_tiled_device(self, dev_imgs: int, B: int, H: int, W: int, conf: float, iou: float, min_area: int,
                         dev_dets: int, dev_counts: int, overlap: int = 128, full_frame: bool = True) -> None:
        t = _tiling(overlap, full_frame)
        check(self.lib, self.lib.lp_run_tiled_device(self._h, C.c_void_p(dev_imgs), B, H, W, C.byref(t), conf, iou, int(min_area),
                                                     C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    # ---- scaled views: any window of a frame, letterboxed at its own scale --------------------
    def view_grid(self, H: int, W: int, tile: int, overlap: int = 0, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
        return view_grid(tile, H, W, overlap, full_frame)

    def view_geometry(self, H: int, W: int, view) -> Dict[str, object]:
        return view_geometry(self.cfg.det_input, H, W, view)

    def run_views(self, images: Sequence[np.ndarray], views, conf: float, iou: float, min_area: int):
        """run_batch with every frame seen through the views (lp_run_views; (x, y, w, h) windows or "full"): same return
        values, per frame."""
        v = _view_array(views)
        return self._run_staged(self.lib.lp_run_views, images, (_ip(v), len(v)), conf, iou, min_area)

    def run_views_device(self, dev_imgs: int, B: int, H: int, W: int, views, conf: float, iou: float, min_area: int,
                         dev_dets: int, dev_counts: int) -> None:
        v = _view_array(views)
        check(self.lib, self.lib.lp_run_views_device(self._h, C.c_void_p(dev_imgs), B, H, W, _ip(v), len(v), conf, iou, int(min_area),
                                                     C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    # ---- mapped views: any lens through a remap table ---------------------------------------------
    def map_add(self, xy, H: int, W: int) -> int:
        """Register the map xy [S, S, 2] float32 (S = det_input; frame positions (x, y) of the view's pixels, cv2.remap's
        convention) for H x W frames (lp_map_add); returns its id: 0, 1, ... in order."""
        xy = np.ascontiguousarray(_map_table(xy), dtype=np.float32)
        if xy.shape[0] != self.cfg.det_input:
            raise ValueError(f"a map of this engine is [{self.cfg.det_input}, {self.cfg.det_input}, 2] (got {xy.shape})")
        mid = C.c_int(-1)
        check(self.lib, self.lib.lp_map_add(self._h, xy.ctypes.data_as(C.POINTER(C.c_float)), int(H), int(W), C.byref(mid)))
        return mid.value

    def map_clear(self) -> None:
        """Drop every map of the engine (lp_map_clear); ids start at 0 again."""
        check(self.lib, self.lib.lp_map_clear(self._h))

    def run_mapped(self, images: Sequence[np.ndarray], views, maps, conf: float, iou: float, min_area: int):
        """run_views with every frame also seen through the maps of the given ids, behind the listed views (lp_run_mapped;
        views may be empty or None): same return values, per frame."""
        v, m = _view_array(views or []), _id_array(maps)
        return self._run_staged(self.lib.lp_run_mapped, images, (_ip(v) if len(v) else None, len(v), _ip(m) if len(m) else None, len(m)),
                                conf, iou, min_area)

    def run_mapped_device(self, dev_imgs: int, B: int, H: int, W: int, views, maps, conf: float, iou: float, min_area: int,
                          dev_dets: int, dev_counts: int) -> None:
        v, m = _view_array(views or []), _id_array(maps)
        check(self.lib, self.lib.lp_run_mapped_device(self._h, C.c_void_p(dev_imgs), B, H, W, _ip(v) if len(v) else None, len(v),
                                                      _ip(m) if len(m) else None, len(m), conf, iou, int(min_area),
                                                      C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    # ---- decoder surfaces in place -------------------------------------------------------------
    def run_surfaces_device(self, surfaces: Sequence[Surface], conf: float, iou: float, min_area: int, dev_dets: int, dev_counts: int,
                            pixfmt: str = "nv12", matrix: str = "bt601") -> None:
        """run_batch_device on decoder surfaces of individual sizes, converted on the device where they lie
        (lp_run_surfaces_device).  Asynchronous: keep the surfaces alive and unwritten until the stream has passed the call."""
        f, arr = surface_format(pixfmt, matrix), surface_array(surfaces)
        check(self.lib, self.lib.lp_run_surfaces_device(self._h, C.byref(f), arr, len(arr), conf, iou, int(min_area),
                                                        C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    def run_views_surfaces_device(self, surfaces: Sequence[Surface], views, conf: float, iou: float, min_area: int, dev_dets: int,
                                  dev_counts: int, pixfmt: str = "nv12", matrix: str = "bt601") -> None:
        """run_views_device on decoder surfaces of one size (lp_run_views_surfaces_device)."""
        f, arr, v = surface_format(pixfmt, matrix), surface_array(surfaces), _view_array(views)
        check(self.lib, self.lib.lp_run_views_surfaces_device(self._h, C.byref(f), arr, len(arr), _ip(v), len(v), conf, iou, int(min_area),
                                                              C.c_void_p(dev_dets), C.c_void_p(dev_counts)))

    def graph_stats(self) -> Dict[str, int]:
        """Captured steps of the engine (lp_graph_stats): entries in the cache, and the calls run eagerly / captured / replayed."""
        n, e, c, r = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
        check(self.lib, self.lib.lp_graph_stats(self._h, C.byref(n), C.byref(e), C.byref(c), C.byref(r)))
        return {"entries": n.value, "eager": e.value, "captures": c.value, "replays": r.value}

    # ---- sign tracking across frames ----------------------------------------------------------
    def tracker_create(self, **cfg) -> None:
        """One tracker per engine (lp_tracker_create); calling it again replaces the tracker and restarts the ids.  Settings are
        lp_track_config's fields: n_streams, max_tracks, iou_match, max_age, min_hits, new_conf, vote_decay, class_gate, motion."""
        c = track_config(**cfg)
        check(self.lib, self.lib.lp_tracker_create(self._h, C.byref(c)))
        self.track_cfg = c
        self.__dict__.pop("inv_cfg", None)   # the inventory belongs to the tracker it was created on
        self.__dict__.pop("ev_cfg", None)    # and the evidence store to the inventory
        self.__dict__.pop("focus_cfg", None)   # and so does the focus plan

    def tracker_destroy(self) -> None:
        check(self.lib, self.lib.lp_tracker_destroy(self._h))
        if hasattr(self, "track_cfg"):
            del self.track_cfg
        self.__dict__.pop("inv_cfg", None)
        self.__dict__.pop("ev_cfg", None)
        self.__dict__.pop("focus_cfg", None)

    def tracker_reset(self, stream: int = -1) -> None:
        """Frees the tracks of one stream (-1: all); ids keep counting.  Asynchronous on the engine's stream."""
        check(self.lib, self.lib.lp_tracker_reset(self._h, int(stream)))

    def _stream_ids(self, stream_ids, B: int):
        if stream_ids is None:
            return None
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        if ids.shape != (B,):
            raise ValueError(f"stream_ids must hold one id per frame ({B}), got shape {ids.shape}")
        return ids

    def track(self, dets: np.ndarray, counts, stream_ids=None) -> np.ndarray:
        """lp_track on host records as run_batch / run_tiled return them: dets [B, max_det] lp_det records, counts [B] ->
        [B, max_det] lp_track records (TRACK_DTYPE), zero beyond a frame's count.  Synchronous."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1, self.cfg.max_det)
        B = d.shape[0]
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (B,):
            raise ValueError(f"counts must hold one count per frame ({B}), got shape {cnt.shape}")
        ids = self._stream_ids(stream_ids, B)
        out = np.zeros((B, self.cfg.max_det), dtype=TRACK_DTYPE)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_track(self._h, d.ctypes.data, cnt.ctypes.data_as(ip), B, None if ids is None else ids.ctypes.data_as(ip),
                                          out.ctypes.data))
        return out

    def track_device(self, dev_dets: int, dev_counts: int, B: int, dev_tracks: int, stream_ids=None) -> None:
        """lp_track_device: consumes the records run_batch_device / run_tiled_device left at dev_dets / dev_counts and writes
        [B * max_det] lp_track records at dev_tracks.  Asynchronous on the engine's stream."""
        ids = self._stream_ids(stream_ids, B)
        check(self.lib, self.lib.lp_track_device(self._h, C.c_void_p(dev_dets), C.c_void_p(dev_counts), int(B),
                                                 None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(dev_tracks)))

    def tracker_snapshot(self, stream: int = 0) -> Dict[str, object]:
        """The live tracks of a stream in slot order, coasting ones included (synchronises): {"tracks": TRACK_STATE_DTYPE records,
        "acc": [n, num_classes] vote accumulators, "next_id", "overflow"}."""
        n, nid, ovf = C.c_int(), C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_tracker_snapshot(self._h, int(stream), None, 0, C.byref(n), None, C.byref(nid), C.byref(ovf)))
        st = np.zeros(n.value, dtype=TRACK_STATE_DTYPE)
        acc = np.zeros((n.value, max(self.cfg.num_classes, 1)), np.float32)
        check(self.lib, self.lib.lp_tracker_snapshot(self._h, int(stream), st.ctypes.data, n.value, C.byref(n), acc.ctypes.data,
                                                     C.byref(nid), C.byref(ovf)))
        return {"tracks": st, "acc": acc, "next_id": nid.value, "overflow": ovf.value}

    # ---- device-side evaluation: detections against ground truth ---------------------------------
    def eval_create(self, **cfg) -> None:
        """One evaluator per engine (lp_eval_create); calling it again replaces it.  Settings: max_gt, max_rows, thr
        (eval_config)."""
        c = eval_config(**cfg)
        check(self.lib, self.lib.lp_eval_create(self._h, C.byref(c)))
        self.eval_cfg = c

    def eval_destroy(self) -> None:
        check(self.lib, self.lib.lp_eval_destroy(self._h))
        self.__dict__.pop("eval_cfg", None)

    def eval_reset(self) -> None:
        """Empties the log and zeroes every counter.  Asynchronous on the engine's stream."""
        check(self.lib, self.lib.lp_eval_reset(self._h))

    def _eval_gts(self, gts, B: int):
        """per-frame ground truth -> ([B, max_gt] GT_DTYPE, [B] int32 counts); the engine refuses what does not fit"""
        if len(gts) != max(B, 0):   # a bad B itself is the engine's to refuse
            raise ValueError(f"gts must hold one list per frame ({B}), got {len(gts)}")
        B = max(B, 0)
        max_gt = self.eval_cfg.max_gt if hasattr(self, "eval_cfg") else _ffi.LP_EVAL_MAX_GT
        recs = [gt_records(g) for g in gts]
        cnt = np.array([len(r) for r in recs], dtype=np.int32)
        table = np.zeros((B, max(max_gt, 1)), dtype=_ffi.GT_DTYPE)
        for b, r in enumerate(recs):
            table[b, :min(len(r), max_gt)] = r[:max_gt]   # a longer list keeps its count: lp_eval* answers LP_ERR_ARG
        return table, cnt

    def evaluate(self, dets: np.ndarray, counts, gts) -> np.ndarray:
        """lp_eval on host records as run_batch / run_tiled return them: dets [B, max_det] lp_det records, counts [B], gts one
        list of (cls, x1, y1, x2, y2) per frame -> [B, max_det] lp_match_rec records (MATCH_DTYPE), zero beyond a frame's count; the
        rows go to the evaluator's log.  Synchronous."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1, self.cfg.max_det)
        B = d.shape[0]
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (B,):
            raise ValueError(f"counts must hold one count per frame ({B}), got shape {cnt.shape}")
        table, gcnt = self._eval_gts(gts, B)
        out = np.zeros((B, self.cfg.max_det), dtype=_ffi.MATCH_DTYPE)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_eval(self._h, d.ctypes.data, cnt.ctypes.data_as(ip), B, table.ctypes.data, gcnt.ctypes.data_as(ip),
                                         out.ctypes.data))
        return out

    def eval_device(self, dev_dets: int, dev_counts: int, B: int, gts, dev_matches: int = 0) -> None:
        """lp_eval_device: consumes the records run_batch_device / run_tiled_device / run_views_device left at dev_dets /
        dev_counts; dev_matches: [B * max_det] lp_match_rec records, or 0 for none.  Asynchronous on the engine's stream: the ground
        truth is read before the call returns."""
        table, gcnt = self._eval_gts(gts, int(B))
        check(self.lib, self.lib.lp_eval_device(self._h, C.c_void_p(dev_dets), C.c_void_p(dev_counts), int(B), table.ctypes.data,
                                                gcnt.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(dev_matches) if dev_matches else None))

    def eval_drain(self) -> Dict[str, object]:
        """The evaluator's log (synchronises, resets nothing): {"rows": EVAL_ROW_DTYPE records in frame order, then record order,
        "gt_per_class": [num_classes] ground-truth boxes seen per class, "frames", "dropped": rows lost to a full log}."""
        n, fr, dr = C.c_int(), C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_eval_drain(self._h, None, 0, C.byref(n), None, C.byref(fr), C.byref(dr)))
        rows = np.zeros(n.value, dtype=_ffi.EVAL_ROW_DTYPE)
        per = np.zeros(max(self.cfg.num_classes, 1), dtype=np.int32)
        check(self.lib, self.lib.lp_eval_drain(self._h, rows.ctypes.data, n.value, C.byref(n), per.ctypes.data_as(C.POINTER(C.c_int)),
                                               C.byref(fr), C.byref(dr)))
        return {"rows": rows, "gt_per_class": per, "frames": fr.value, "dropped": dr.value}

    # ---- class distributions: top-k per detection and the distribution vote --------------------
    def topk_enable(self, k: int) -> None:
        """lp_topk_enable: k in 1..8 = every pipeline call also leaves the k most probable classes of every detection in the
        engine's lp_topk buffer (topk_read, topk_buffer); 0 = off (the default)."""
        check(self.lib, self.lib.lp_topk_enable(self._h, int(k)))
        self.topk_k = int(k)

    def topk_buffer(self) -> Tuple[int, int]:
        """(device address of the [max_batch * max_det] lp_topk records, k); the address is stable for the engine's life."""
        p, k = C.c_void_p(), C.c_int()
        check(self.lib, self.lib.lp_topk_buffer(self._h, C.byref(p), C.byref(k)))
        return int(p.value or 0), k.value

    def topk_read(self, B: int) -> np.ndarray:
        """lp_topk_read (synchronises): the last pipeline call's records of its first B frames, (B, max_det) TOPK_DTYPE --
        cls (8,) i4 and prob (8,) f4, parallel to the lp_det records; unused entries cls = -1, prob = 0."""
        out = np.zeros((max(int(B), 0), self.cfg.max_det), dtype=TOPK_DTYPE)
        check(self.lib, self.lib.lp_topk_read(self._h, out.ctypes.data, int(B)))
        return out

    def topk_select(self, p, k: int) -> np.ndarray:
        """lp_topk_select (host only): the selection rule on one distribution p [nc] -> one TOPK_DTYPE record."""
        return topk_select(p, k)

    def _topk_records(self, topk, B: int) -> np.ndarray:
        t = np.ascontiguousarray(topk, dtype=TOPK_DTYPE).reshape(-1, self.cfg.max_det)
        if t.shape[0] != B:
            raise ValueError(f"topk must hold max_det records per frame ({B} frames), got shape {np.shape(topk)}")
        return t

    def track_topk(self, dets: np.ndarray, counts, topk, stream_ids=None) -> np.ndarray:
        """lp_track_topk: track() with the distribution vote -- every detection votes with its lp_topk record (topk [B, max_det]
        TOPK_DTYPE, as topk_read returns them) instead of (cls_class, cls_conf).  Synchronous."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1, self.cfg.max_det)
        B = d.shape[0]
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (B,):
            raise ValueError(f"counts must hold one count per frame ({B}), got shape {cnt.shape}")
        t = self._topk_records(topk, B)
        ids = self._stream_ids(stream_ids, B)
        out = np.zeros((B, self.cfg.max_det), dtype=TRACK_DTYPE)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_track_topk(self._h, d.ctypes.data, cnt.ctypes.data_as(ip), t.ctypes.data, B,
                                               None if ids is None else ids.ctypes.data_as(ip), out.ctypes.data))
        return out

    def track_topk_device(self, dev_dets: int, dev_counts: int, dev_topk: int, B: int, dev_tracks: int, stream_ids=None) -> None:
        """lp_track_topk_device: track_device() with the distribution vote; dev_topk is topk_buffer()'s address or any device
        buffer of [B * max_det] lp_topk records.  Asynchronous on the engine's stream."""
        ids = self._stream_ids(stream_ids, B)
        check(self.lib, self.lib.lp_track_topk_device(self._h, C.c_void_p(dev_dets), C.c_void_p(dev_counts), C.c_void_p(dev_topk), int(B),
                                                      None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(dev_tracks)))

    def test_topk(self, probs, img, slot, B: int) -> np.ndarray:
        """lp_test_topk: probs [R, num_classes] as the classifier would leave them and the ROI list (img[r], slot[r]) through the
        clear + select launches for B frames -> (B, max_det) TOPK_DTYPE records.  Needs top-k on."""
        nc = max(self.cfg.num_classes, 1)
        p = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1, nc)
        i, s = np.ascontiguousarray(img, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
        if i.shape != (len(p),) or s.shape != (len(p),):
            raise ValueError("img and slot must hold one entry per row of probs")
        out = np.zeros((max(int(B), 0), self.cfg.max_det), dtype=TOPK_DTYPE)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        check(self.lib, self.lib.lp_test_topk(self._h, p.ctypes.data_as(fp), len(p), i.ctypes.data_as(ip), s.ctypes.data_as(ip), int(B),
                                              out.ctypes.data))
        return out

    # ---- crop quality: sharpness and exposure per detection ------------------------------------
    def quality_enable(self, on: bool = True) -> None:
        """lp_quality_enable: on = every pipeline call also leaves an lp_quality record (sharpness, luma mean and variance, clipped
        shares) of every classified detection's crop in the engine's buffer (quality_read, quality_buffer); off is the default."""
        check(self.lib, self.lib.lp_quality_enable(self._h, int(on)))
        self.quality_on = bool(on)

    def quality_buffer(self) -> int:
        """device address of the [max_batch * max_det] lp_quality records; stable for the engine's life."""
        p = C.c_void_p()
        check(self.lib, self.lib.lp_quality_buffer(self._h, C.byref(p)))
        return int(p.value or 0)

    def quality_read(self, B: int) -> np.ndarray:
        """lp_quality_read (synchronises): the last pipeline call's records of its first B frames, (B, max_det) QUALITY_DTYPE,
        parallel to the lp_det records; a detection without a crop has the empty record (sharpness -1, flags 0)."""
        out = np.zeros((max(int(B), 0), self.cfg.max_det), dtype=QUALITY_DTYPE)
        check(self.lib, self.lib.lp_quality_read(self._h, out.ctypes.data, int(B)))
        return out

    def test_quality(self, B: int) -> np.ndarray:
        """lp_test_quality: the ROI list and crops test_set_rois installed through the clear + measure launches for B frames ->
        (B, max_det) QUALITY_DTYPE records.  Needs quality on."""
        out = np.zeros((max(int(B), 0), self.cfg.max_det), dtype=QUALITY_DTYPE)
        check(self.lib, self.lib.lp_test_quality(self._h, int(B), out.ctypes.data))
        return out

    def inventory_set_rank(self, rank) -> None:
        """lp_inventory_set_rank: "config" (lp_inventory_config's best, the default) or "sharpness" (a track's best sighting is
        its sharpest crop; needs quality on), or the enum value.  inventory_create restores "config"."""
        if isinstance(rank, str):
            if rank not in INVENTORY_RANKS:
                raise ValueError(f"rank must be one of {tuple(INVENTORY_RANKS)}, got {rank!r}")
            rank = INVENTORY_RANKS[rank]
        check(self.lib, self.lib.lp_inventory_set_rank(self._h, int(rank)))

    # ---- focus views: tracker-chosen windows and a sweep ---------------------------------------
    def focus_create(self, **cfg) -> None:
        """One focus plan per tracker (lp_focus_create); calling it again replaces it.  Settings are lp_focus_config's fields:
        slots, side_min, side_max, margin, small_px, border, sweep, sweep_overlap."""
        c = focus_config(**cfg)
        check(self.lib, self.lib.lp_focus_create(self._h, C.byref(c)))
        self.focus_cfg = c

    def focus_destroy(self) -> None:
        check(self.lib, self.lib.lp_focus_destroy(self._h))
        self.__dict__.pop("focus_cfg", None)

    def _focus_slots(self) -> int:
        """the slot count of the plan (without one the library refuses the call: any size will do)"""
        return int(self.focus_cfg.slots) if hasattr(self, "focus_cfg") else 16

    def focus_plan(self, heights, widths, stream_ids=None, advance: bool = True) -> np.ndarray:
        """lp_focus_plan: the windows the plan chooses now for B frames of heights[b] x widths[b] -> int32 [B, slots, 4]
        {x, y, w, h}, empty slots all zero.  advance=False leaves the cursor and the unserved counter alone.  Synchronous."""
        hs, ws = np.ascontiguousarray(heights, dtype=np.int32), np.ascontiguousarray(widths, dtype=np.int32)
        B = hs.shape[0]
        if hs.shape != (B,) or ws.shape != (B,):
            raise ValueError(f"heights and widths must hold one size per frame, got shapes {hs.shape} and {ws.shape}")
        ids = self._stream_ids(stream_ids, B)
        out = np.zeros((B, self._focus_slots(), 4), np.int32)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_focus_plan(self._h, B, hs.ctypes.data_as(ip), ws.ctypes.data_as(ip),
                                               None if ids is None else ids.ctypes.data_as(ip), out.ctypes.data_as(ip), int(bool(advance))))
        return out

    def focus_state(self, stream: int = 0) -> Dict[str, int]:
        """{"cursor", "unserved"} of a stream (synchronises)."""
        c, u = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_focus_state(self._h, int(stream), C.byref(c), C.byref(u)))
        return {"cursor": c.value, "unserved": u.value}

    def run_focus(self, images: Sequence[np.ndarray], conf: float, iou: float, min_area: int, stream_ids=None):
        """run_batch with every frame seen through the whole frame and its plan's windows (lp_run_focus): run_batch's return
        values per frame, then the windows used, int32 [B, slots, 4]."""
        B = len(images)
        ids = self._stream_ids(stream_ids, B)
        views = np.zeros((B, self._focus_slots(), 4), np.int32)
        ip = C.POINTER(C.c_int)

        def fn(h, ptrs, hs, ws, n, *rest):
            return self.lib.lp_run_focus(h, ptrs, hs, ws, n, None if ids is None else ids.ctypes.data_as(ip), *rest, views.ctypes.data_as(ip))

        return self._run_staged(fn, images, (), conf, iou, min_area) + (views,)

    def run_focus_device(self, dev_imgs: int, B: int, H: int, W: int, conf: float, iou: float, min_area: int,
                         dev_dets: int, dev_counts: int, stream_ids=None, dev_views: int = 0) -> None:
        """lp_run_focus_device; dev_views (0: not wanted) receives [B * slots * 4] int32.  Asynchronous on the engine's stream."""
        ids = self._stream_ids(stream_ids, B)
        check(self.lib, self.lib.lp_run_focus_device(self._h, C.c_void_p(dev_imgs), B, H, W,
                                                     None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int)), conf, iou,
                                                     int(min_area), C.c_void_p(dev_dets), C.c_void_p(dev_counts),
                                                     C.c_void_p(dev_views) if dev_views else None))

    # ---- sign inventory: one record and best crop per finished track ---------------------------
    def inventory_create(self, **cfg) -> None:
        """One inventory per tracker (lp_inventory_create); calling it again replaces it.  Settings are lp_inventory_config's fields:
        max_signs, keep_crops, best ("area" | "det_conf" | "cls_conf" or the enum value), min_hits."""
        c = inventory_config(**cfg)
        check(self.lib, self.lib.lp_inventory_create(self._h, C.byref(c)))
        self.inv_cfg = c
        self.__dict__.pop("ev_cfg", None)

    def inventory_destroy(self) -> None:
        check(self.lib, self.lib.lp_inventory_destroy(self._h))
        self.__dict__.pop("inv_cfg", None)
        self.__dict__.pop("ev_cfg", None)

    def inventory(self, dets: np.ndarray, counts, tracks: np.ndarray, stream_ids=None, crops: bool = False) -> None:
        """lp_inventory on host records: dets [B, max_det] lp_det, counts [B], tracks [B, max_det] lp_track as track() returned
        them.  crops: frames 0..B-1 are those of the engine's last pipeline call, whose crops are attached.  Synchronous."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE).reshape(-1, self.cfg.max_det)
        B = d.shape[0]
        t = np.ascontiguousarray(tracks, dtype=TRACK_DTYPE).reshape(-1, self.cfg.max_det)
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (B,) or t.shape[0] != B:
            raise ValueError(f"counts and tracks must hold {B} frames, got shapes {cnt.shape} and {t.shape}")
        ids = self._stream_ids(stream_ids, B)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_inventory(self._h, d.ctypes.data, cnt.ctypes.data_as(ip), t.ctypes.data, B,
                                              None if ids is None else ids.ctypes.data_as(ip), int(crops)))

    def inventory_device(self, dev_dets: int, dev_counts: int, dev_tracks: int, B: int, stream_ids=None, crops: bool = False) -> None:
        """lp_inventory_device: the buffers and stream ids of the preceding track_device call.  Asynchronous on the engine's stream."""
        ids = self._stream_ids(stream_ids, B)
        check(self.lib, self.lib.lp_inventory_device(self._h, C.c_void_p(dev_dets), C.c_void_p(dev_counts), C.c_void_p(dev_tracks), int(B),
                                                     None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int)), int(crops)))

    def inventory_flush(self, stream: int = -1) -> None:
        """Closes every open entry of one stream (-1: all) into the log with LP_SIGN_FLUSHED.  Asynchronous."""
        check(self.lib, self.lib.lp_inventory_flush(self._h, int(stream)))

    def inventory_drain(self, crops: bool = True):
        """The logged signs since the last drain (synchronises, empties the log): (SIGN_DTYPE records [n], crops [n, S, S, 3] uint8
        RGB or None, dropped)."""
        n, dropped = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_inventory_drain(self._h, None, None, 0, C.byref(n), C.byref(dropped)))
        S = self.cfg.cls_input
        signs = np.zeros(n.value, dtype=SIGN_DTYPE)
        pix = np.zeros((n.value, S, S, 3), np.uint8) if crops else None
        check(self.lib, self.lib.lp_inventory_drain(self._h, signs.ctypes.data, None if pix is None else pix.ctypes.data, n.value, C.byref(n),
                                                    C.byref(dropped)))
        return signs, pix, dropped.value

    def inventory_open(self, stream: int = 0) -> np.ndarray:
        """The open entries of a stream in slot order as they would be logged now (synchronises): SIGN_DTYPE records."""
        n = C.c_int()
        check(self.lib, self.lib.lp_inventory_open(self._h, int(stream), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=SIGN_DTYPE)
        check(self.lib, self.lib.lp_inventory_open(self._h, int(stream), out.ctypes.data, n.value, C.byref(n)))
        return out

    # ---- evidence store: a context picture of each sign's best sighting ---------------------------
    def evidence_create(self, size: int = 128, scale: float = 2.0) -> None:
        """One evidence store per inventory (lp_evidence_create); calling it again replaces it.  size: side E of the BGR pictures
        (a multiple of 16 in 32..256); scale: the window's side is scale x the box's longer side (1..16)."""
        c = evidence_config(size=size, scale=scale)
        check(self.lib, self.lib.lp_evidence_create(self._h, C.byref(c)))
        self.ev_cfg = c

    def evidence_destroy(self) -> None:
        check(self.lib, self.lib.lp_evidence_destroy(self._h))
        self.__dict__.pop("ev_cfg", None)

    def inventory_drain_evidence(self, crops: bool = True):
        """inventory_drain with the pictures: (signs [n], crops [n, S, S, 3] RGB or None, evidence [n, E, E, 3] uint8 BGR,
        windows [n, 4] int32 {x, y, w, h}, dropped); evidence and windows are zeros for a sign without LP_SIGN_HAS_EVIDENCE."""
        n, dropped = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_inventory_drain_evidence(self._h, None, None, None, None, 0, C.byref(n), C.byref(dropped)))
        S, E = self.cfg.cls_input, self.ev_cfg.size
        signs = np.zeros(n.value, dtype=SIGN_DTYPE)
        pix = np.zeros((n.value, S, S, 3), np.uint8) if crops else None
        ev, win = np.zeros((n.value, E, E, 3), np.uint8), np.zeros((n.value, 4), np.int32)
        check(self.lib, self.lib.lp_inventory_drain_evidence(self._h, signs.ctypes.data, None if pix is None else pix.ctypes.data, ev.ctypes.data,
                                                             win.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        return signs, pix, ev, win, dropped.value

    def evidence_open(self, stream: int = 0):
        """The pictures [n, E, E, 3] and windows [n, 4] of a stream's open entries in slot order, parallel to inventory_open
        (synchronises)."""
        n = C.c_int()
        check(self.lib, self.lib.lp_evidence_open(self._h, int(stream), None, None, 0, C.byref(n)))
        E = self.ev_cfg.size
        ev, win = np.zeros((n.value, E, E, 3), np.uint8), np.zeros((n.value, 4), np.int32)
        check(self.lib, self.lib.lp_evidence_open(self._h, int(stream), ev.ctypes.data, win.ctypes.data, n.value, C.byref(n)))
        return ev, win

    def test_set_frames(self, frames: np.ndarray) -> None:
        """lp_test_set_frames: host BGR frames [B, H, W, 3] of one size, as lp_run_batch would leave them in the handle."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim != 4 or f.shape[3] != 3:
            raise ValueError(f"frames must be [B, H, W, 3], got {f.shape}")
        check(self.lib, self.lib.lp_test_set_frames(self._h, f.ctypes.data, f.shape[0], f.shape[1], f.shape[2]))

    def test_set_rois(self, crops: np.ndarray, img, slot) -> None:
        """lp_test_set_rois: a ROI list (img[r], slot[r]) and its crops [R, S, S, 3] as a pipeline call would leave them."""
        S = self.cfg.cls_input
        c = np.ascontiguousarray(crops, dtype=np.uint8).reshape(-1, S, S, 3)
        i, s = np.ascontiguousarray(img, dtype=np.int32), np.ascontiguousarray(slot, dtype=np.int32)
        if i.shape != (len(c),) or s.shape != (len(c),):
            raise ValueError("img and slot must hold one entry per crop")
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_test_set_rois(self._h, c.ctypes.data, i.ctypes.data_as(ip), s.ctypes.data_as(ip), len(c)))

    def debug_rois(self):
        """lp_debug_rois: the last pipeline call's (crops [R, S, S, 3] uint8 RGB, img [R], slot [R]) (synchronises)."""
        n = C.c_int()
        check(self.lib, self.lib.lp_debug_rois(self._h, None, None, None, 0, C.byref(n)))
        S, R = self.cfg.cls_input, n.value
        crops, img, slot = np.zeros((R, S, S, 3), np.uint8), np.zeros(R, np.int32), np.zeros(R, np.int32)
        ip = C.POINTER(C.c_int)
        check(self.lib, self.lib.lp_debug_rois(self._h, crops.ctypes.data, img.ctypes.data_as(ip), slot.ctypes.data_as(ip), R, C.byref(n)))
        return crops, img, slot

    def roi_overflow(self) -> Tuple[int, int]:
        """(classified, kept) of the last run_batch_device call (synchronises): kept > classified means max_rois was too small."""
        a, b = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_roi_overflow(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def classify(self, rois: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        imgs, ptrs, hs, ws = self._img_args(rois)
        R = len(imgs)
        ids = (C.c_int * R)()
        probs = np.empty((R, self.cfg.num_classes), np.float32)
        check(self.lib, self.lib.lp_classify(self._h, ptrs, hs, ws, R, ids, probs.ctypes.data_as(C.POINTER(C.c_float))))
        return np.array(ids[:], dtype=np.int64), probs

    # ---- streams / profiling -------------------------------------------------------------------
    def set_stream(self, stream_handle: int) -> None:
        check(self.lib, self.lib.lp_set_stream(self._h, C.c_void_p(stream_handle)))

    def synchronize(self) -> None:
        check(self.lib, self.lib.lp_synchronize(self._h))

    def profile_next(self, enable: bool = True) -> None:
        check(self.lib, self.lib.lp_profile_next(self._h, int(enable)))

    def profile_read(self) -> List[dict]:
        n = C.c_int()
        cap = 512
        buf = (LpKernelTime * cap)()
        check(self.lib, self.lib.lp_profile_read(self._h, buf, cap, C.byref(n)))
        return [dict(name=buf[i].name.decode(), layer=buf[i].layer.decode(), ms=buf[i].ms, flops=buf[i].flops,
                     bytes=buf[i].bytes) for i in range(min(cap, n.value))]

    # ---- test hooks ----------------------------------------------------------------------------
    def debug_blob(self, name: str, batch: int = 1) -> np.ndarray:
        """Blob ``name`` of the first ``batch`` images of the last ``detect_raw`` call (at most the handle's capacity)."""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_debug_blob(self._h, name.encode(), None, 0, C.byref(c), C.byref(h), C.byref(w)))
        out = np.empty((batch, c.value, h.value, w.value), np.float32)
        check(self.lib, self.lib.lp_debug_blob(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size,
                                               C.byref(c), C.byref(h), C.byref(w)))
        return out

    def test_conv(self, x, w, bias, stride=1, act=0, res=None, impl=0) -> np.ndarray:
        fp = C.POINTER(C.c_float)
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        N, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        y = np.empty((N, Cout, Ho, Wo), np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        r = None if res is None else np.ascontiguousarray(res, np.float32)
        check(self.lib, self.lib.lp_test_conv(self._h, impl, x.ctypes.data_as(fp), N, Cin, H, W, w.ctypes.data_as(fp),
                                              None if b is None else b.ctypes.data_as(fp), Cout, k, stride, act,
                                              None if r is None else r.ctypes.data_as(fp), y.ctypes.data_as(fp)))
        return y

    def test_postprocess(self, out0, orig_shape, ratio, pad, conf, iou, min_area: int = -1, max_det: int = 0, with_rects: bool = False):
        """filter + NMS (+ ROI clip / area filter when min_area >= 0) on a host out0 [4+nc, A].  Returns the records, or
        (records, int rects [n,4], pre-filter count) with ``with_rects``."""
        fp = C.POINTER(C.c_float)
        o = np.ascontiguousarray(out0, np.float32)
        nc, A = o.shape[0] - 4, o.shape[1]
        dets = np.zeros(A, dtype=DET_DTYPE)
        rects = np.zeros((A, 4), dtype=np.int32)
        cnt, num = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_test_postprocess(self._h, o.ctypes.data_as(fp), nc, A, int(orig_shape[0]), int(orig_shape[1]),
                                                     float(ratio), float(pad[0]), float(pad[1]), float(conf), float(iou),
                                                     int(min_area), int(max_det), dets.ctypes.data,
                                                     rects.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cnt), C.byref(num)))
        if with_rects:
            return dets[:cnt.value], rects[:cnt.value], num.value
        return dets[:cnt.value]

    def test_nms_boxes(self, boxes, scores, classes, orig_shape, iou, min_area: int = -1, max_det: int = 0):
        """NMS + ROI clip / area filter on host xyxy boxes -> (records, int rects [n,4], pre-filter count)."""
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        sc = np.ascontiguousarray(scores, np.float32)
        n = len(b)
        cl = None if classes is None else np.ascontiguousarray(classes, np.int32)
        dets = np.zeros(max(n, 1), dtype=DET_DTYPE)
        rects = np.zeros((max(n, 1), 4), dtype=np.int32)
        cnt, num = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_test_nms_boxes(self._h, b.ctypes.data_as(fp), sc.ctypes.data_as(fp),
                                                   None if cl is None else cl.ctypes.data_as(ip), n, int(orig_shape[0]),
                                                   int(orig_shape[1]), float(iou), int(min_area), int(max_det), dets.ctypes.data,
                                                   rects.ctypes.data_as(ip), C.byref(cnt), C.byref(num)))
        return dets[:cnt.value], rects[:cnt.value], num.value

    def test_nms_views(self, boxes, scores, classes, views, anchors, n_views, orig_shape, iou, min_area: int = -1, max_det: int = 0):
        """The frame NMS of tiled inference on host candidates tagged (view, anchor) -> (records, int rects [n,4], pre-filter count)."""
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        sc = np.ascontiguousarray(scores, np.float32)
        n = len(b)
        cl = None if classes is None else np.ascontiguousarray(classes, np.int32)
        vw, an = np.ascontiguousarray(views, np.int32), np.ascontiguousarray(anchors, np.int32)
        dets = np.zeros(max(n, 1), dtype=DET_DTYPE)
        rects = np.zeros((max(n, 1), 4), dtype=np.int32)
        cnt, num = C.c_int(), C.c_int()
        check(self.lib, self.lib.lp_test_nms_views(self._h, b.ctypes.data_as(fp), sc.ctypes.data_as(fp),
                                                   None if cl is None else cl.ctypes.data_as(ip), vw.ctypes.data_as(ip),
                                                   an.ctypes.data_as(ip), n, int(n_views), int(orig_shape[0]), int(orig_shape[1]),
                                                   float(iou), int(min_area), int(max_det), dets.ctypes.data, rects.ctypes.data_as(ip),
                                                   C.byref(cnt), C.byref(num)))
        return dets[:cnt.value], rects[:cnt.value], num.value

    def test_tile_views(self, img: np.ndarray, overlap: int = 128, full_frame: bool = True, byte_offset: int = 0) -> np.ndarray:
        """The gathered views of one frame (uploaded byte_offset bytes past an aligned address) -> uint8 [n_views, S, S, 3]."""
        a = _as_bgr(img)
        S = self.cfg.det_input
        t = _tiling(overlap, full_frame)
        n = C.c_int()
        check(self.lib, self.lib.lp_test_tile_views(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(t), int(byte_offset), None,
                                                    0, C.byref(n)))
        out = np.empty((n.value, S, S, 3), np.uint8)
        check(self.lib, self.lib.lp_test_tile_views(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(t), int(byte_offset),
                                                    out.ctypes.data, n.value, C.byref(n)))
        return out

    def test_view_windows(self, img: np.ndarray, views, byte_offset: int = 0) -> np.ndarray:
        """The gathered views of one frame (uploaded byte_offset bytes past an aligned address) -> uint8 [n_views, S, S, 3]."""
        a = _as_bgr(img)
        S = self.cfg.det_input
        v = _view_array(views)
        out = np.empty((len(v), S, S, 3), np.uint8)
        check(self.lib, self.lib.lp_test_view_windows(self._h, a.ctypes.data, a.shape[0], a.shape[1], _ip(v), len(v), int(byte_offset),
                                                      out.ctypes.data, len(v)))
        return out

    def test_map_views(self, img: np.ndarray, maps, byte_offset: int = 0) -> np.ndarray:
        """The mapped gather alone: one frame (uploaded byte_offset bytes past an aligned address, the buffer ending with its last
        byte) through the maps of the given ids -> uint8 [n_maps, S, S, 3]."""
        a = _as_bgr(img)
        S = self.cfg.det_input
        m = _id_array(maps)
        out = np.empty((len(m), S, S, 3), np.uint8)
        check(self.lib, self.lib.lp_test_map_views(self._h, a.ctypes.data, a.shape[0], a.shape[1], _ip(m), len(m), int(byte_offset),
                                                   out.ctypes.data, len(m)))
        return out

    def test_map_boxes(self, map_id: int, boxes) -> np.ndarray:
        """The candidate kernel alone: view boxes [n, 4] through map map_id -> frame boxes [n, 4] float32."""
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
        out = np.zeros_like(b)
        fp = C.POINTER(C.c_float)
        check(self.lib, self.lib.lp_test_map_boxes(self._h, int(map_id), b.ctypes.data_as(fp), len(b), out.ctypes.data_as(fp)))
        return out

    def test_convert_frames(self, frames: np.ndarray, B: int, H: int, W: int, matrix: str = "bt601", pitch: int = 0, uv_offset: int = 0,
                            frame_stride: int = 0, byte_offset: int = 0) -> np.ndarray:
        """The NV12 converter alone: the bytes of B frames of one layout -> uint8 BGR [B, H, W, 3]."""
        f = _frame_format("nv12", matrix, pitch, uv_offset, frame_stride)
        _, nb = frame_layout(H, W, "nv12", matrix, pitch, uv_offset, frame_stride)
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        need = (B - 1) * (frame_stride or nb) + nb
        if a.size < need:
            raise ValueError(f"{B} frames of this layout are {need} bytes, got {a.size}")
        out = np.empty((B, H, W, 3), np.uint8)
        check(self.lib, self.lib.lp_test_convert_frames(self._h, a.ctypes.data, int(B), int(H), int(W), C.byref(f), int(byte_offset),
                                                        out.ctypes.data))
        return out

    def test_convert_surfaces(self, surfaces: Sequence[Surface], pixfmt: str = "nv12", matrix: str = "bt601") -> List[np.ndarray]:
        """The surface converter alone (lp_test_convert_surfaces): device surfaces -> one uint8 BGR [H, W, 3] array each."""
        surfaces = list(surfaces)
        f, arr = surface_format(pixfmt, matrix), surface_array(surfaces)
        surfaces_check(surfaces, pixfmt, matrix)   # the sizes below are the output's: nothing unchecked sizes a buffer
        nb = [s.height * s.width * 3 for s in surfaces]
        out = np.empty(sum(nb), np.uint8)
        check(self.lib, self.lib.lp_test_convert_surfaces(self._h, C.byref(f), arr, len(arr), out.ctypes.data))
        offs = np.concatenate([[0], np.cumsum(nb)])
        return [out[offs[i]:offs[i + 1]].reshape(s.height, s.width, 3) for i, s in enumerate(surfaces)]

    def test_roi_resize(self, rois: Sequence[np.ndarray]) -> np.ndarray:
        imgs, ptrs, hs, ws = self._img_args(rois)
        S = self.cfg.cls_input
        out = np.empty((len(imgs), S, S, 3), np.uint8)
        check(self.lib, self.lib.lp_test_roi_resize(self._h, ptrs, hs, ws, len(imgs), out.ctypes.data))
        return out

    def test_roi_resize_rects(self, frame: np.ndarray, rects) -> np.ndarray:
        """The ROI resize of (x1, y1, x2, y2) rectangles of one BGR frame -> uint8 RGB [R, S, S, 3]."""
        a = _as_bgr(frame)
        rc = np.ascontiguousarray(np.array(rects, dtype=np.int32).reshape(-1, 4))
        S = self.cfg.cls_input
        out = np.empty((len(rc), S, S, 3), np.uint8)
        check(self.lib, self.lib.lp_test_roi_resize_rects(self._h, a.ctypes.data, a.shape[0], a.shape[1], _ip(rc), len(rc), out.ctypes.data))
        return out

    def test_letterbox(self, img: np.ndarray, per_pixel: bool = False):
        """The letterbox alone -> (uint8 [SH, SW, 3], ratio, (pad_w, pad_h)); per_pixel: the per-pixel kernel instead of the
        launcher's choice (the tiled kernel where its LDS rows fit)."""
        a = _as_bgr(img)
        out = np.empty((*self.det_hw, 3), np.uint8)
        r, pw, ph = C.c_float(), C.c_float(), C.c_float()
        check(self.lib, self.lib.lp_test_letterbox_kernel(self._h, a.ctypes.data, a.shape[0], a.shape[1], int(bool(per_pixel)),
                                                          out.ctypes.data, C.byref(r), C.byref(pw), C.byref(ph)))
        return out, r.value, (pw.value, ph.value)


# ==================== reference-compatible surface ====================
@dataclass
class PipelineMetrics:
    """Same fields as the reference dataclass (e2e.py:34-62)."""
    t_detection: float = 0.0
    t_roi_extract: float = 0.0
    t_classification: float = 0.0
    t_postprocess: float = 0.0
    t_total: float = 0.0
    fps: float = 0.0
    num_detections: int = 0
    det_confidence_avg: float = 0.0
    cls_confidence_avg: float = 0.0
    cpu_percent: float = 0.0
    memory_mb: float = 0.0
    temperature: float = 0.0
    precision: float = 0.0
    recall: float = 0.0
    f1: float = 0.0
    level: str = "HIP(MI355X)"


_SYSM_CACHE = [0.0, (0.0, 0.0, 0.0)]
_SYSM_PERIOD_S = 0.25


def _system_metrics():
    """cpu_percent / memory_mb / temperature as the reference samples them after each run (e2e.py:509-516).  One sample costs
    ~1.2 ms (psutil + a sysfs read): more than a 64-image batch takes on the GPU.  The reference's calls are 50+ ms apart; here
    the sample is refreshed at most every 0.25 s and calls in between report the last one."""
    now = time.monotonic()
    if now - _SYSM_CACHE[0] < _SYSM_PERIOD_S:
        return _SYSM_CACHE[1]
    cpu = mem = temp = 0.0
    try:
        import psutil
        cpu = float(psutil.cpu_percent())
        mem = float(psutil.Process().memory_info().rss) / 1024 / 1024
    except Exception:  # noqa: BLE001 - psutil missing: fields stay 0 like the reference's temperature fallback
        pass
    try:
        with open("/sys/class/thermal/thermal_zone0/temp") as f:
            temp = float(f.read()) / 1000.0
    except Exception:  # noqa: BLE001
        pass
    _SYSM_CACHE[0], _SYSM_CACHE[1] = now, (cpu, mem, temp)
    return cpu, mem, temp


def _empty_detect():
    # the reference returns float64 empties here (e2e.py:264,292-294)
    return np.empty((0, 4)), np.empty((0,)), np.empty((0,))


class NCNNDetector:
    """e2e.py:195-316.  ``use_gpu``/``num_threads`` are accepted and ignored (the detector always
    runs on the HIP device)."""

    def __init__(self, param_path: str, bin_path: Optional[str], input_size=640, use_gpu: bool = False, num_threads: int = 4,
                 input_name: str = "in0", output_name: str = "out0", *, precision: str = "fp16", max_batch: int = 1,
                 max_det: int = 300, device: int = 0, pixel_format: str = "bgr", csc_matrix: str = "bt601",
                 _engine: Optional[Engine] = None):
        self.input_size = input_size
        self.input_name = input_name
        self.output_name = output_name
        print("[HIP Detector] Loading model...")
        print(f"  {'Param' if bin_path is not None else 'ONNX'}: {param_path}")
        if bin_path is not None:
            print(f"  Bin: {bin_path}")
        self.engine = _engine or Engine(precision=precision, max_batch=max_batch, max_det=max_det, det_input=input_size,
                                        device=device)
        if _engine is None:
            self.engine.set_input_format(pixel_format, csc_matrix)
        try:
            self.engine.load_detector(param_path, bin_path)
        except _ffi.LitepiError as e:  # e2e.py:213-216 raises RuntimeError on load failure
            raise RuntimeError(str(e)) from e
        print(f"  Device: HIP:{self.engine.cfg.device} ({self.engine.precision})")
        print("  Input size: {}x{}".format(*reversed(det_input_hw(input_size))))

    def detect_batch(self, images: Sequence[np.ndarray], conf_threshold: float = 0.5, iou_threshold: float = 0.45):
        try:
            dets, counts = self.engine.detect(images, conf_threshold, iou_threshold)
        except _ffi.LitepiError as e:
            # the reference returns empty arrays when the ENGINE call fails (extract != 0, e2e.py:309-310): that is a HIP
            # runtime failure here.  Misuse (batch over capacity, unsupported shapes, model not loaded) is raised.
            if e.code != _ffi.LP_ERR_HIP:
                raise
            print(f"[HIP Detector] engine failure, returning no detections: {e}")
            return [_empty_detect() for _ in images]
        out = []
        for i, n in enumerate(counts):
            if n == 0:
                out.append(_empty_detect())
                continue
            d = dets[i, :n]
            boxes = np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], axis=1).astype(np.float32)
            out.append((boxes, d["det_conf"].astype(np.float32), d["det_class"].astype(np.int64)))
        return out

    def detect(self, image: np.ndarray, conf_threshold: float = 0.5, iou_threshold: float = 0.45):
        return self.detect_batch([image], conf_threshold, iou_threshold)[0]


class ONNXDetector(NCNNDetector):
    """NCNNDetector for an ONNX export of the detector (what the reference's notebooks run through ONNX Runtime): same
    ``detect`` / ``detect_batch``, same results as the NCNN export of that model."""

    def __init__(self, onnx_path: str, input_size=640, use_gpu: bool = False, num_threads: int = 4, input_name: str = "images",
                 output_name: str = "output0", **kw):
        super().__init__(onnx_path, None, input_size, use_gpu, num_threads, input_name, output_name, **kw)


def load_classifier_state(model_path: Optional[str], num_classes: int, arch: str = "shufflenetv2"):
    """torch is used only to READ the checkpoint (weights_only: nothing from the file is executed).
    Returns (state_dict, loaded_flag); a missing/unreadable file gives seeded random weights and a
    warning, like the reference's silent random-init fallback (e2e.py:337-343)."""
    import torch

    if model_path and os.path.exists(model_path):
        try:
            sd = torch.load(model_path, map_location="cpu", weights_only=True)
            if isinstance(sd, dict) and "state_dict" in sd:
                sd = sd["state_dict"]
            print(f"Loaded classifier weights from {model_path}")
            return sd, True
        except Exception as e:  # noqa: BLE001 - mirror the reference's catch-all
            print(f"WARNING: could not load classifier weights ({e}); the classifier stays RANDOM-INIT")
    else:
        print(f"WARNING: classifier weights {model_path!r} not found; the classifier stays RANDOM-INIT")
    return {"resnet18": random_resnet18_state, "mobilenetv2": random_mobilenetv2_state, "efficientnet": random_efficientnet_state,
            "shufflenetv2": random_shufflenet_state}[arch](num_classes), False


def random_shufflenet_state(num_classes: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random ShuffleNetV2 x1.0 state_dict with torchvision's key names and shapes."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}

    def conv(name, co, ci, k):
        sd[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * (1.7 / (ci * k * k)) ** 0.5).astype(np.float32)

    def bn(name, c):
        sd[name + ".weight"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.75, 1.25, c).astype(np.float32)

    conv("conv1.0", 24, 3, 3)
    bn("conv1.1", 24)
    inp = 24
    for stage, rep, oup in (("stage2", 4, 116), ("stage3", 8, 232), ("stage4", 4, 464)):
        bf = oup // 2
        for r in range(rep):
            p = f"{stage}.{r}."
            if r == 0:
                conv(p + "branch1.0", inp, 1, 3); bn(p + "branch1.1", inp)
                conv(p + "branch1.2", bf, inp, 1); bn(p + "branch1.3", bf)
                conv(p + "branch2.0", bf, inp, 1)
            else:
                conv(p + "branch2.0", bf, bf, 1)
            bn(p + "branch2.1", bf)
            conv(p + "branch2.3", bf, 1, 3); bn(p + "branch2.4", bf)
            conv(p + "branch2.5", bf, bf, 1); bn(p + "branch2.6", bf)
        inp = oup
    conv("conv5.0", 1024, 464, 1)
    bn("conv5.1", 1024)
    sd["fc.weight"] = (rng.standard_normal((num_classes, 1024)) * (1.0 / 1024) ** 0.5).astype(np.float32)
    sd["fc.bias"] = (rng.standard_normal(num_classes) * 0.1).astype(np.float32)
    return sd


def _rand_helpers(rng, sd, gain):
    def conv(name, co, ci, k):
        sd[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * (gain / (ci * k * k)) ** 0.5).astype(np.float32)

    def bn(name, c):
        sd[name + ".weight"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
    return conv, bn


def random_mobilenetv2_state(num_classes: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random mobilenet_v2 state_dict with torchvision's key names and shapes (features.i.conv.*, classifier.1.*)."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    conv, bn = _rand_helpers(rng, sd, 2.0)
    conv("features.0.0", 32, 3, 3); bn("features.0.1", 32)
    inp, idx = 32, 1
    for t, c, n, s in ([1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2], [6, 320, 1, 1]):
        for _ in range(n):
            p, hid, li = f"features.{idx}.conv.", inp * t, 0
            if t != 1:
                conv(p + "0.0", hid, inp, 1); bn(p + "0.1", hid)
                li = 1
            conv(p + f"{li}.0", hid, 1, 3); bn(p + f"{li}.1", hid)
            conv(p + f"{li + 1}", c, hid, 1); bn(p + f"{li + 2}", c)
            inp = c
            idx += 1
    conv("features.18.0", 1280, inp, 1); bn("features.18.1", 1280)
    sd["classifier.1.weight"] = (rng.standard_normal((num_classes, 1280)) * (1.0 / 1280) ** 0.5).astype(np.float32)
    sd["classifier.1.bias"] = (rng.standard_normal(num_classes) * 0.1).astype(np.float32)
    return sd


def random_efficientnet_state(num_classes: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random efficientnet_b0 state_dict with torchvision's key names and shapes (features.s.r.block.*, classifier.1.*)."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    conv, bn = _rand_helpers(rng, sd, 2.0)
    conv("features.0.0", 32, 3, 3); bn("features.0.1", 32)
    cfg = [(1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
           (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1)]
    for si, (e, k, s, i, o, n) in enumerate(cfg):
        for r in range(n):
            inp = i if r == 0 else o
            p, exp, li = f"features.{si + 1}.{r}.block.", inp * e, 0
            if e != 1:
                conv(p + "0.0", exp, inp, 1); bn(p + "0.1", exp)
                li = 1
            conv(p + f"{li}.0", exp, 1, k); bn(p + f"{li}.1", exp)
            sq = max(1, inp // 4)
            conv(p + f"{li + 1}.fc1", sq, exp, 1); sd[p + f"{li + 1}.fc1.bias"] = (rng.standard_normal(sq) * 0.1).astype(np.float32)
            conv(p + f"{li + 1}.fc2", exp, sq, 1); sd[p + f"{li + 1}.fc2.bias"] = (rng.standard_normal(exp) * 0.1).astype(np.float32)
            conv(p + f"{li + 2}.0", o, exp, 1); bn(p + f"{li + 2}.1", o)
    conv("features.8.0", 1280, 320, 1); bn("features.8.1", 1280)
    sd["classifier.1.weight"] = (rng.standard_normal((num_classes, 1280)) * (1.0 / 1280) ** 0.5).astype(np.float32)
    sd["classifier.1.bias"] = (rng.standard_normal(num_classes) * 0.1).astype(np.float32)
    return sd


def random_resnet18_state(num_classes: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random resnet18 state_dict with torchvision's key names and shapes."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}

    def conv(name, co, ci, k):
        sd[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * (1.4 / (ci * k * k)) ** 0.5).astype(np.float32)

    def bn(name, c):
        sd[name + ".weight"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[name + ".bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.75, 1.25, c).astype(np.float32)

    conv("conv1", 64, 3, 7)
    bn("bn1", 64)
    cin = 64
    for L, width in enumerate((64, 128, 256, 512)):
        for r in range(2):
            p = f"layer{L + 1}.{r}"
            stride = 2 if (L > 0 and r == 0) else 1
            conv(p + ".conv1", width, cin, 3); bn(p + ".bn1", width)
            conv(p + ".conv2", width, width, 3); bn(p + ".bn2", width)
            if stride != 1 or cin != width:
                conv(p + ".downsample.0", width, cin, 1); bn(p + ".downsample.1", width)
            cin = width
    sd["fc.weight"] = (rng.standard_normal((num_classes, 512)) * (1.0 / 512) ** 0.5).astype(np.float32)
    sd["fc.bias"] = (rng.standard_normal(num_classes) * 0.1).astype(np.float32)
    return sd


class PyTorchClassifier:
    """e2e.py:350-396 (name kept for drop-in use; the model runs in HIP, not torch)."""

    def __init__(self, model_path: str, arch: str, num_classes: int = 58, input_size: int = 64, device: str = "cpu", *,
                 precision: str = "fp16", max_rois: int = 1024, conv_impl: int = 0, _engine: Optional[Engine] = None):
        if arch not in CLS_ARCHS:
            raise ValueError(f"Unknown architecture: {arch}")   # as build_classifier, e2e.py:334
        self.input_size = input_size
        self.num_classes = num_classes
        self.arch = arch
        print(f"[HIP Classifier] Loading {arch} model...")
        print(f"  Model: {model_path}")
        self.engine = _engine or Engine(precision=precision, max_batch=1, max_det=max_rois, num_classes=num_classes,
                                        cls_input=input_size, max_rois=max_rois, cls_arch=arch, conv_impl=conv_impl)
        if self.engine.cls_arch != arch:
            raise ValueError(f"the engine was created for {self.engine.cls_arch}, not {arch}")
        sd, self.weights_loaded = load_classifier_state(model_path, num_classes, arch)
        self.state_dict = sd   # (HybridPipeline's upload lanes load the same weights)
        self.engine.load_classifier(sd)
        print(f"  Architecture: {arch}")
        print(f"  Input size: {input_size}x{input_size}")
        print(f"  Num classes: {num_classes}")

    def predict_batch(self, images: List[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        if len(images) == 0:
            return np.array([]), np.array([])  # e2e.py:380-381
        ids, probs = self.engine.classify(images)
        return ids, probs


class HybridPipeline:
    """e2e.py:399-531 with one extra method, ``run_batch``.  Detector and classifier share one
    device handle, so detections never leave the GPU between the two stages."""

    def __init__(self, detector_param: str, detector_bin: Optional[str], classifier_path: str, classifier_arch: str,
                 num_classes: int = 58, det_input_size=640, cls_input_size: int = 64, use_gpu_detector: bool = False,
                 detector_threads: int = 4, classifier_device: str = "cpu", batch_size: int = 8, *, precision: str = "fp16",
                 max_batch: int = 1, max_det: int = 300, device: int = 0, max_rois: int = 0, numerics: str = "e2e",
                 tile_overlap: Optional[int] = None, tile_full_frame: bool = True, pixel_format: str = "bgr",
                 csc_matrix: str = "bt601", track: bool = False, track_config: Optional[Dict] = None, inventory=False,
                 views=None, view_tile: Optional[int] = None, view_overlap: int = 0, view_full_frame: bool = True,
                 focus: Optional[int] = None, focus_config: Optional[Dict] = None, view_match: Optional[str] = None,
                 view_merge: Optional[str] = None, view_match_thr: Optional[float] = None, evidence=None,
                 topk: Optional[int] = None, track_vote: str = "top1", quality: bool = False, view_maps=None,
                 view_maps_frame: Optional[Tuple[int, int]] = None, evaluate=False):
        """detector_param, detector_bin: an NCNN .param / .bin pair, or an .onnx file and None.
        inventory: True or a dict of lp_inventory_config's fields (max_signs, keep_crops, best, min_hits): every tracked call
        also feeds the engine's sign inventory, while the handle still holds that call's classifier crops; drain_signs() returns
        the finished signs.  Needs track.
        evidence: an int E or a dict {"size": E, "scale": s} (lp_evidence_config): the inventory also keeps an E x E BGR picture
        of the surroundings of every sign's best sighting, cut from the native frame (Engine.evidence_create); drain_signs()
        dicts then gain evidence and evidence_window.  Needs inventory (with keep_crops).
        track: run_batch also tracks the detections across calls (lp_track on the engine's tracker, created here with
        track_config: lp_track_config's fields); every result dict then gains track_id, track_hits, track_age, track_cls,
        track_cls_conf and track_confirmed.  The frames of consecutive calls are a sequence (per stream id).
        pixel_format: "bgr" = HxWx3 arrays (the reference's cv2 images); "nv12" = video frames as (H * 3 // 2, W) arrays,
        converted on the device with csc_matrix ("bt601" = cv2's COLOR_YUV2BGR_NV12 constants, "bt709" = HD video).
        tile_overlap: None = every frame is letterboxed to det_input (the reference's behaviour); an int = tiled inference
        (lp_run_tiled): frames larger than det_input are also seen as native-resolution crops overlapping by that many pixels,
        with the letterboxed whole frame as an extra view when tile_full_frame.
        views: scaled views (lp_run_views): a list of (x, y, w, h) source windows and / or "full", each letterboxed into the
        detector batch at its own scale and applied to every frame; or view_tile (with view_overlap, view_full_frame): the
        window grid of lp_view_grid for every frame's size.  Mutually exclusive with each other and with tile_overlap.
        focus: K = focus views (lp_run_focus): every frame is seen through the whole frame and K windows the engine's tracker
        chooses on the device, the free ones swept over a window grid (focus_config: lp_focus_config's other fields).  Needs
        track and a max_batch of at least 1 + K; mutually exclusive with tile_overlap, views and view_tile.  The windows of
        the last run_batch are in last_focus_views.
        view_maps, view_maps_frame: mapped views (lp_run_mapped): a list of remap tables xy [S, S, 2] float32 (S = det_input_size;
        litepi.lens builds some) for frames of view_maps_frame = (H, W); every frame is seen through `views` (if given) and then
        through every map, and boxes come back in frame coordinates.  Needs a square det_input_size; mutually exclusive with
        tile_overlap, view_tile and focus.
        view_match, view_merge, view_match_thr: how one frame's views are merged (Engine.set_view_merge): "ios" matches a box a
        view border cut with the whole box it lies in, "union" emits the box around a keeper and everything it absorbed.  Valid
        only together with tile_overlap, views, view_tile or focus.
        det_input_size: an int (square) or (rows, columns), e.g. (384, 640) for 16:9 video; tile_overlap, views, view_tile and
        focus need a square.
        topk: K in 1..8 (Engine.topk_enable): every result dict gains "cls_topk", the [(class, prob), ...] of the detection's K
        most probable classes in descending order ([] for an unclassified detection); cls_topk[0] is (cls_class, cls_conf).
        track_vote: "top1" = a detection adds (cls_class, cls_conf) to its track's vote; "distribution" = it adds its K most
        probable classes, each with its probability (lp_track_topk).  "distribution" needs track and topk >= 1.
        quality: True (Engine.quality_enable) = every result dict gains "sharpness", "luma_mean", "clip_lo" and "clip_hi" of the
        detection's classifier crop (floats; None for a detection without a crop).  inventory=dict(best="sharpness") ranks a
        track's sightings by that sharpness instead of an lp_best (Engine.inventory_set_rank) and switches quality on.
        evaluate: True or a dict of eval_config's settings (max_gt, max_rows, thr): the engine gets an evaluator
        (Engine.eval_create), run_batch(gts=...) matches every engine call's records against the frames' ground truth on the
        device, and evaluation() returns the metrics of everything fed so far.  Not available with the upload lanes."""
        self.evaluate = bool(evaluate) or isinstance(evaluate, dict)
        if self.evaluate:
            if eval_config_check(eval_config(**(evaluate if isinstance(evaluate, dict) else {}))) != 0:
                raise ValueError(f"evaluate {evaluate!r}: max_gt in 1..{_ffi.LP_EVAL_MAX_GT}, max_rows >= 1, thr without a NaN")
            if int(os.environ.get("LITEPI_DROPIN_LANES", "1")) > 1:
                raise ValueError("evaluate: the upload lanes run on other handles than the evaluator's; unset LITEPI_DROPIN_LANES")
        self.quality, self._inv_rank, inv_settings = check_quality_options(quality, inventory)
        self.topk = check_topk_options(topk, track_vote, bool(track) or track_config is not None)
        self.track_vote = track_vote
        merge_set = [n for n, v in (("view_match", view_match), ("view_merge", view_merge), ("view_match_thr", view_match_thr)) if v is not None]
        if merge_set and all(v is None for v in (tile_overlap, views, view_tile, focus, view_maps)):
            raise ValueError(f"{', '.join(merge_set)} need one of tile_overlap, views, view_tile or focus: a frame seen through one "
                             f"letterboxed view has nothing to merge")
        if merge_set:
            vm = view_merge_config(view_match or "iou", view_merge or "nms", 0.0 if view_match_thr is None else view_match_thr)
            if view_merge_check(vm) != 0:
                raise ValueError(f"view_match_thr {view_match_thr!r} outside [0, 1)")
        for name, value in (("tile_overlap", tile_overlap), ("views", views), ("view_tile", view_tile), ("focus", focus),
                            ("view_maps", view_maps)):
            if value is not None:
                _square_only(det_input_size, name)
        self.tile_overlap, self.tile_full_frame = tile_overlap, bool(tile_full_frame)
        if sum(x is not None for x in (tile_overlap, views, view_tile)) > 1:
            raise ValueError("tile_overlap, views and view_tile are mutually exclusive")
        self.views = None if views is None else [tuple(r) for r in _view_array(views).tolist()]
        if self.views is not None and not self.views:
            raise ValueError("views needs at least one view")
        self.view_tile, self.view_overlap, self.view_full_frame = view_tile, int(view_overlap), bool(view_full_frame)
        self.view_mode = self.views is not None or view_tile is not None
        self.view_maps, self.view_maps_frame, self._map_ids = None, None, []
        if view_maps is not None:
            for name, value in (("tile_overlap", tile_overlap), ("view_tile", view_tile), ("focus", focus)):
                if value is not None:
                    raise ValueError(f"view_maps is mutually exclusive with {name}")
            if view_maps_frame is None or len(tuple(view_maps_frame)) != 2 or min(int(v) for v in view_maps_frame) < 1:
                raise ValueError("view_maps needs view_maps_frame = (H, W), the size of the frames the maps belong to")
            side = det_input_hw(det_input_size)[1]
            self.view_maps = [np.ascontiguousarray(_map_table(m, "a map of view_maps"), dtype=np.float32) for m in view_maps]
            if not self.view_maps or len(self.view_maps) > _ffi.LP_MAP_MAX:
                raise ValueError(f"view_maps holds 1..{_ffi.LP_MAP_MAX} maps (got {len(self.view_maps)})")
            for m in self.view_maps:
                if m.shape[0] != side:
                    raise ValueError(f"a map of view_maps is [{side}, {side}, 2] for det_input_size {side} (got {m.shape})")
                if np.isnan(m).any():
                    raise ValueError("a map of view_maps holds a NaN")
            self.view_maps_frame = (int(view_maps_frame[0]), int(view_maps_frame[1]))
            self.view_mode = True
        elif view_maps_frame is not None:
            raise ValueError("view_maps_frame needs view_maps")
        self.focus = None if focus is None else int(focus)
        if self.focus is not None:
            if tile_overlap is not None or self.view_mode:
                raise ValueError("focus is mutually exclusive with tile_overlap, views and view_tile")
            if not (track or track_config is not None):
                raise ValueError("focus needs a pipeline constructed with track=True or a track_config")
            if max_batch < 1 + self.focus:
                raise ValueError(f"focus = {self.focus} needs max_batch >= {1 + self.focus} (it is {max_batch})")
            if "slots" in (focus_config or {}):
                raise ValueError("focus_config: the number of slots is the focus argument")
            if int(os.environ.get("LITEPI_DROPIN_LANES", "1")) > 1:
                raise ValueError("focus: the upload lanes run on other handles than the tracker's; unset LITEPI_DROPIN_LANES")
        elif focus_config is not None:
            raise ValueError("focus_config needs focus")
        self.inventory = bool(inventory) or isinstance(inventory, dict)
        if self.inventory and not (track or track_config is not None):
            raise ValueError("inventory needs a pipeline constructed with track=True or a track_config")
        if self.inventory and int(os.environ.get("LITEPI_DROPIN_LANES", "1")) > 1:
            raise ValueError("inventory: the upload lanes keep their crops on other handles; unset LITEPI_DROPIN_LANES")
        self.evidence = None
        if evidence is not None and evidence is not False:
            if not self.inventory:
                raise ValueError("evidence needs a pipeline constructed with inventory=True")
            ev = dict(evidence) if isinstance(evidence, dict) else {"size": int(evidence)}
            if evidence_config_check(evidence_config(**ev)) != 0:
                raise ValueError(f"evidence {evidence!r}: size must be a multiple of 16 in 32..256 and scale in 1..16")
            if isinstance(inventory, dict) and not int(inventory.get("keep_crops", 1)):
                raise ValueError("evidence needs an inventory with keep_crops")
            self.evidence = ev
        print("\n" + "=" * 70)
        print("HYBRID PIPELINE: HIP Detector + HIP Classifier (MI355X)")
        print("=" * 70)
        self.engine = Engine(precision=precision, max_batch=max_batch, max_det=max_det, num_classes=num_classes,
                             det_input=det_input_size, cls_input=cls_input_size, device=device, max_rois=max_rois,
                             numerics=numerics, cls_arch=classifier_arch if classifier_arch in CLS_ARCHS else "shufflenetv2")
        self.engine.set_input_format(pixel_format, csc_matrix)
        self.pixel_format, self.csc_matrix = pixel_format, csc_matrix
        if self.topk:
            self.engine.topk_enable(self.topk)
        self._topk_parts: List[np.ndarray] = []   # the lp_topk records of a run_batch's engine calls, in frame order
        if self.quality:
            self.engine.quality_enable(True)
        self._quality_parts: List[np.ndarray] = []   # the lp_quality records likewise
        if merge_set:
            self.engine.set_view_merge(view_match or "iou", view_merge or "nms", 0.0 if view_match_thr is None else view_match_thr)
        self.detector = NCNNDetector(detector_param, detector_bin, det_input_size, use_gpu_detector, detector_threads,
                                     _engine=self.engine)
        self.classifier = PyTorchClassifier(classifier_path, classifier_arch, num_classes, cls_input_size, classifier_device,
                                            _engine=self.engine)
        self.batch_size = batch_size  # kept for signature parity: all ROIs of a call are classified in one pass
        self.track = bool(track)
        if self.track or track_config is not None:
            self.engine.tracker_create(**(track_config or {}))
        if self.view_maps is not None:
            self._map_ids = [self.engine.map_add(m, *self.view_maps_frame) for m in self.view_maps]
        self.last_focus_views: List = []
        if self.focus is not None:
            self.engine.focus_create(slots=self.focus, **(focus_config or {}))
        self.signs_dropped = 0
        if self.inventory:
            self.engine.inventory_create(**inv_settings)
            if self._inv_rank != "config":
                self.engine.inventory_set_rank(self._inv_rank)
        if self.evidence is not None:
            self.engine.evidence_create(**self.evidence)
        if self.evaluate:   # absent: the engine is constructed exactly as before
            self.engine.eval_create(**(evaluate if isinstance(evaluate, dict) else {}))
        # ---- upload lanes (an experiment kept behind LITEPI_DROPIN_LANES=<n>, off by default: measured SLOWER, 3.2-3.6 ms per
        # 64-frame call against 2.7-2.9 for one handle -- four 16-frame passes cost 1.4 ms of kernels instead of 0.9 and four
        # sets of copy workers fight over the cores; walking a large batch in chunks inside lp_run_batch gained nothing either
        # and was removed).  Lanes are further handles of max_batch / lanes images each
        # (own stream, staging buffer, copy workers, the same models); a call's images are dealt to them in contiguous slices and
        # every slice runs lp_run_batch on its lane from a worker thread (ctypes drops the GIL).  Results do not depend on the
        # split (tests/test_gpu_device_path.py compares both).
        self._lanes: List[Engine] = []
        self._lane_pool = None
        n_lanes = int(os.environ.get("LITEPI_DROPIN_LANES", "1"))
        if n_lanes > 1 and pixel_format != "bgr":
            raise ValueError("LITEPI_DROPIN_LANES: the upload lanes take packed BGR frames only; unset it for pixel_format " + repr(pixel_format))
        if n_lanes > 1 and max_batch >= 2 * n_lanes:
            from concurrent.futures import ThreadPoolExecutor
            lane_cap = -(-max_batch // n_lanes)
            lane_rois = max_rois if max_rois <= 0 else -(-max_rois // n_lanes)
            for _ in range(n_lanes):
                e = Engine(precision=precision, max_batch=lane_cap, max_det=max_det, num_classes=num_classes, det_input=det_input_size,
                           cls_input=cls_input_size, device=device, max_rois=lane_rois, numerics=numerics, cls_arch=self.engine.cls_arch)
                e.load_detector(detector_param, detector_bin)
                e.load_classifier(self.classifier.state_dict)
                if self.topk:
                    e.topk_enable(self.topk)
                if self.quality:
                    e.quality_enable(True)
                self._lanes.append(e)
            self._lane_pool = ThreadPoolExecutor(max_workers=n_lanes, thread_name_prefix="litepi-lane")
            self._lane_cap = lane_cap
        print("\nPipeline ready!")
        print("=" * 70 + "\n")

    def close(self) -> None:
        if self._lane_pool is not None:
            self._lane_pool.shutdown(wait=True)
            self._lane_pool = None
        for e in self._lanes:
            e.close()
        self._lanes = []
        self.engine.close()

    def _run_lanes(self, images, conf, iou, min_area):
        """run_batch's engine call over the upload lanes: contiguous slices, results concatenated in image order."""
        B, n = len(images), len(self._lanes)
        per = -(-B // n)
        slices = [(k, k * per, min(B, (k + 1) * per)) for k in range(n) if k * per < B]

        def one(arg):
            k, lo, hi = arg
            e = self._lanes[k]
            d, c, nd, t = e.run_batch(images[lo:hi], conf, iou, min_area)
            return d, c, nd, t, e.last_det_conf_avg, (e.topk_read(hi - lo) if self.topk else None), (e.quality_read(hi - lo) if self.quality else None)

        parts = list(self._lane_pool.map(one, slices))
        dets = np.concatenate([p[0] for p in parts], 0)
        counts = np.concatenate([p[1] for p in parts])
        num_det = np.concatenate([p[2] for p in parts])
        timing = LpTiming()
        for f in ("t_detection", "t_roi_extract", "t_classification", "t_total"):   # the lanes run side by side: the longest one
            setattr(timing, f, max(getattr(p[3], f) for p in parts))
        self.engine.last_det_conf_avg = np.concatenate([p[4] for p in parts])
        if self.topk:
            self._topk_parts = [p[5] for p in parts]
        if self.quality:
            self._quality_parts = [p[6] for p in parts]
        return dets, counts, num_det, timing

    def _run_grouped(self, images, feed, verb, frame_views, call):
        """run_batch's engine call in tiled mode and with scaled views.  frame_views(fh, fw) -> (key, n): the frame's n views
        and what the engine call needs to know of them.  Consecutive frames go to one call(frames, key) while they share the
        key, the sum of their views fits max_batch and their ROIs fit max_rois (at most max_det per frame).  Tiled frames all
        share one key, so only the sum counts; frames under scaled views share a key when they share the view list, and
        then the sum is frames x views.  Results concatenated in frame order, stage times summed over the calls.
        feed(dets, counts, first_frame) is called behind every engine call."""
        cfg = self.engine.cfg
        cap = cfg.max_batch
        max_frames = max(1, (cfg.max_rois if cfg.max_rois > 0 else cfg.max_batch * cfg.max_det) // cfg.max_det)
        groups, cur, cur_key, used = [], [], None, 0
        for img in images:
            fh, fw = self.engine.frame_hw(img)
            key, n = frame_views(fh, fw)
            if n > cap:
                raise ValueError(f"a {fw}x{fh} frame {verb} {n} views, more than max_batch = {cap}")
            if cur and (key != cur_key or used + n > cap or len(cur) >= max_frames):
                groups.append((cur, cur_key))
                cur, used = [], 0
            cur.append(img)
            cur_key = key
            used += n
        if cur:
            groups.append((cur, cur_key))
        return self._run_groups(groups, feed, call)

    def _run_groups(self, groups, feed, call):
        """the engine calls of _run_grouped / _run_focus over (frames, key) groups, results concatenated in frame order"""
        parts, done = [], 0
        for g, key in groups:
            d, c, nd, t = call(g, key)
            parts.append((d, c, nd, t, self.engine.last_det_conf_avg))
            if self.topk:   # the buffer holds the last engine call's records: read before the next call replaces them
                self._topk_parts.append(self.engine.topk_read(len(g)))
            if self.quality:
                self._quality_parts.append(self.engine.quality_read(len(g)))
            if feed is not None:
                feed(d[:len(g)], c[:len(g)], done)
            done += len(g)
        timing = LpTiming()
        for f in ("t_detection", "t_roi_extract", "t_classification", "t_total"):
            setattr(timing, f, sum(getattr(p[3], f) for p in parts))
        self.engine.last_det_conf_avg = np.concatenate([p[4] for p in parts])
        return (np.concatenate([p[0] for p in parts], 0), np.concatenate([p[1] for p in parts]),
                np.concatenate([p[2] for p in parts]), timing)

    def _run_tiled(self, images, conf, iou, min_area, feed=None):
        """lp_run_tiled calls of consecutive frames whose views fit max_batch"""
        S, ov, full = self.engine.cfg.det_input, self.tile_overlap, self.tile_full_frame
        return self._run_grouped(images, feed, "needs", lambda fh, fw: (None, len(tile_grid(S, fh, fw, ov, full))),
                                 lambda g, _: self.engine.run_tiled(g, conf, iou, min_area, ov, full))

    def _run_views(self, images, conf, iou, min_area, feed=None):
        """lp_run_views calls of consecutive frames that share a view list (view_tile: the grid of their size) and fit max_batch;
        with view_maps, lp_run_mapped calls on the list and the maps"""
        def frame_views(fh, fw):
            if self.view_maps is not None:
                vs = self.views or []
                return vs, len(vs) + len(self._map_ids)
            vs = self.views if self.views is not None else view_grid(self.view_tile, fh, fw, self.view_overlap, self.view_full_frame)
            return vs, len(vs)
        if self.view_maps is not None:
            return self._run_grouped(images, feed, "has", frame_views,
                                     lambda g, vs: self.engine.run_mapped(g, vs, self._map_ids, conf, iou, min_area))
        return self._run_grouped(images, feed, "has", frame_views, lambda g, vs: self.engine.run_views(g, vs, conf, iou, min_area))

    def _run_focus(self, images, conf, iou, min_area, feed, ids):
        """lp_run_focus calls of consecutive frames: at most one frame per stream in a call, so that every frame is planned from
        the tracker state of the frame before it (the feed runs behind every call), and 1 + focus views per frame within
        max_batch.  The windows every frame was seen through are kept in last_focus_views, [slots][4] per frame."""
        cfg = self.engine.cfg
        per_call = min(cfg.max_batch // (1 + self.focus),
                       max(1, (cfg.max_rois if cfg.max_rois > 0 else cfg.max_batch * cfg.max_det) // cfg.max_det))
        groups, cur, cur_ids = [], [], []
        for k, img in enumerate(images):
            s = 0 if ids is None else int(ids[k])
            if cur and (s in cur_ids or len(cur) >= per_call):
                groups.append((cur, cur_ids))
                cur, cur_ids = [], []
            cur.append(img)
            cur_ids.append(s)
        if cur:
            groups.append((cur, cur_ids))
        self.last_focus_views = []

        def call(g, g_ids):
            d, c, nd, t, views = self.engine.run_focus(g, conf, iou, min_area, stream_ids=g_ids)
            self.last_focus_views += views.tolist()
            return d, c, nd, t
        return self._run_groups(groups, feed, call)

    def _track_call(self, dets, counts, ids, topk):
        """one tracker call under the pipeline's vote: lp_track, or lp_track_topk on the frames' lp_topk records"""
        if self.track_vote == "distribution":
            return self.engine.track_topk(dets, counts, topk, ids)
        return self.engine.track(dets, counts, ids)

    def _track(self, dets, counts, stream_ids, topk=None):
        """the call's records through the engine's tracker, at most max_batch frames per lp_track call, in frame order"""
        B, cap = len(counts), self.engine.cfg.max_batch
        ids = None if stream_ids is None else np.asarray(stream_ids, dtype=np.int32)
        parts = [self._track_call(dets[i:i + cap], counts[i:i + cap], None if ids is None else ids[i:i + cap],
                                  None if topk is None else topk[i:i + cap]) for i in range(0, B, cap)]
        return np.concatenate(parts, 0)

    def _feed(self, dets, counts, stream_ids, first, topk=None):
        """one engine call's records through the tracker and, while the handle still holds that call's crops, the inventory"""
        cnt = np.asarray(counts, dtype=np.int32)
        ids = None if stream_ids is None else stream_ids[first:first + len(cnt)]
        tracks = self._track_call(dets, cnt, ids, topk)
        if self.inventory:
            self.engine.inventory(dets, cnt, tracks, ids, crops=bool(self.engine.inv_cfg.keep_crops))
        return tracks

    def drain_signs(self, flush: bool = False) -> List[Dict]:
        """The signs finished since the last call, one dict per track: stream, track_id, first_frame, last_frame, hits, cls,
        cls_conf (the final vote), bbox, det_class, best_frame (of the best sighting), crop (the classifier's RGB input crop of
        the best sighting, or None), flushed; with evidence also evidence (the [E, E, 3] BGR picture of the best sighting's
        surroundings, or None) and evidence_window (x, y, w, h in the frame, or None).  flush: first close every open track
        (the end of a video).  The signs lost to a full log are counted in signs_dropped."""
        if not self.inventory:
            raise ValueError("drain_signs needs a pipeline constructed with inventory=True")
        if flush:
            self.engine.inventory_flush(-1)
        pics = wins = None
        if self.evidence is not None:
            signs, crops, pics, wins, dropped = self.engine.inventory_drain_evidence(crops=bool(self.engine.inv_cfg.keep_crops))
        else:
            signs, crops, dropped = self.engine.inventory_drain(crops=bool(self.engine.inv_cfg.keep_crops))
        self.signs_dropped += dropped
        boxes = np.stack([signs["x1"], signs["y1"], signs["x2"], signs["y2"]], 1).astype(int).tolist()
        out = []
        for k, s in enumerate(signs.tolist()):
            rec = dict(zip(signs.dtype.names, s))
            has = crops is not None and bool(rec["flags"] & _ffi.LP_SIGN_HAS_CROP)
            out.append({"stream": rec["stream"], "track_id": rec["track_id"], "first_frame": rec["first_frame"], "last_frame": rec["last_frame"],
                        "hits": rec["hits"], "cls": rec["voted_class"], "cls_conf": rec["voted_conf"], "bbox": tuple(boxes[k]),
                        "det_class": rec["det_class"], "best_frame": rec["best_frame"], "crop": crops[k].copy() if has else None,
                        "flushed": bool(rec["flags"] & _ffi.LP_SIGN_FLUSHED)})
            if pics is not None:
                pic = bool(rec["flags"] & _ffi.LP_SIGN_HAS_EVIDENCE)
                out[-1]["evidence"] = pics[k].copy() if pic else None
                out[-1]["evidence_window"] = tuple(int(v) for v in wins[k]) if pic else None
        return out

    def run_batch(self, images: Sequence[np.ndarray], conf_threshold: float = 0.5, iou_threshold: float = 0.45,
                  min_area: int = 100, stream_ids=None, track: Optional[bool] = None, gts=None,
                  evaluate: Optional[bool] = None) -> List[Tuple[List[Dict], PipelineMetrics]]:
        """stream_ids: the tracker stream of every image (None: all stream 0); track: None = the constructor's setting.
        gts: one list of (cls, x1, y1, x2, y2) per image: the engine's evaluator is fed behind every engine call of the batch
        (evaluation() returns the metrics).  evaluate: None = the constructor's setting; False = this call is not scored (a
        warm-up or a timing pass) and takes no gts.  evaluate without gts, or gts without evaluate, is a ValueError.
        With focus views, track=False still plans the windows from the tracker's state (and moves the sweep) but feeds it nothing.
        In tiled mode (and with scaled views) tracker and inventory are fed behind every engine call of the batch: if a later call of the batch
        fails, they have consumed the frames of the earlier ones although the caller gets no result for the batch."""
        do_eval = self.evaluate if evaluate is None else bool(evaluate)
        if do_eval and not self.evaluate:
            raise ValueError("run_batch(evaluate=True) needs a pipeline constructed with evaluate=True or an evaluator configuration")
        check_eval_options(do_eval, gts, len(images))
        do_track = self.track if track is None else bool(track)
        if do_track and not hasattr(self.engine, "track_cfg"):
            raise ValueError("run_batch(track=True) needs a pipeline constructed with track=True or a track_config")
        # track (and inventory) are fed per engine call; the tracker's result does not depend on the split
        fed, ids = [], None
        if do_track and stream_ids is not None:
            ids = self.engine._stream_ids(stream_ids, len(images))

        def feed(d, c, first):   # a failure of the tracker, the inventory or the evaluator is never taken for an engine failure below
            try:
                if do_track:
                    fed.append(self._feed(d, c, ids, first, self._topk_parts[-1] if self.topk else None))
                if do_eval:   # frame-level records of this engine call against its frames' ground truth
                    self.engine.evaluate(d, np.asarray(c, dtype=np.int32), gts[first:first + len(c)])
            except _ffi.LitepiError as e:
                e.from_feed = True
                raise
        self._topk_parts = []
        self._quality_parts = []
        t0 = time.perf_counter()
        try:
            if self.focus is not None:
                dets, counts, num_det, timing = self._run_focus(list(images), conf_threshold, iou_threshold, min_area, feed if (do_track or do_eval) else None,
                                                                None if stream_ids is None else self.engine._stream_ids(stream_ids, len(images)))
            elif self.tile_overlap is not None:
                dets, counts, num_det, timing = self._run_tiled(list(images), conf_threshold, iou_threshold, min_area, feed if (do_track or do_eval) else None)
            elif self.view_mode:
                dets, counts, num_det, timing = self._run_views(list(images), conf_threshold, iou_threshold, min_area, feed if (do_track or do_eval) else None)
            elif self._lanes and len(images) >= 32 and len(images) <= self._lane_cap * len(self._lanes):
                dets, counts, num_det, timing = self._run_lanes(list(images), conf_threshold, iou_threshold, min_area)
            else:
                dets, counts, num_det, timing = self.engine.run_batch(images, conf_threshold, iou_threshold, min_area)
                if self.topk:
                    self._topk_parts.append(self.engine.topk_read(len(images)))
                if self.quality:
                    self._quality_parts.append(self.engine.quality_read(len(images)))
                if do_eval:
                    try:
                        self.engine.evaluate(dets[:len(images)], np.asarray(counts[:len(images)], dtype=np.int32), gts)
                    except _ffi.LitepiError as e:
                        e.from_feed = True
                        raise
        except _ffi.LitepiError as e:
            if e.code != _ffi.LP_ERR_HIP or getattr(e, "from_feed", False):  # misuse / capacity errors are raised, only an engine failure yields "nothing found"
                raise
            print(f"[HIP Pipeline] engine failure, returning no detections: {e}")
            return [([], PipelineMetrics()) for _ in images]
        tracks = None
        topk = np.concatenate(self._topk_parts, 0) if self.topk else None
        quality = np.concatenate(self._quality_parts, 0) if self.quality else None
        if do_track:
            B = len(images)
            if self.tile_overlap is not None or self.view_mode or self.focus is not None:
                tracks = np.concatenate(fed, 0)
            elif self.inventory:   # one engine call on this handle
                tracks = self._feed(dets[:B], counts[:B], ids, 0, topk)
            else:
                tracks = self._track(dets[:B], np.asarray(counts[:B], dtype=np.int32), stream_ids, topk)
        wall_ms = (time.perf_counter() - t0) * 1000.0   # t_total ends here; system metrics are sampled after it (e2e.py:505-516)
        conf_avg = self.engine.last_det_conf_avg
        sysm = _system_metrics()
        B = len(images)
        # every used record of the batch decoded in ONE pass (a Python loop over structured-array fields cost 5 us per
        # detection: 2 ms for the ~400 results of a 64-image batch): the float box is truncated to int like the reference's
        # tuple(box.astype(int)) (e2e.py:522), float32 fields become Python floats of the same value
        cnt_a = np.asarray(counts[:B], dtype=np.int64)
        cnt = cnt_a.tolist()
        used = dets[:B][np.arange(dets.shape[1])[None, :] < cnt_a[:, None]]
        boxes = list(map(tuple, np.stack([used["x1"], used["y1"], used["x2"], used["y2"]], 1).astype(int).tolist()))
        det_cls, cls_cls = used["det_class"].tolist(), used["cls_class"].tolist()
        det_cf, cls_cf = used["det_conf"].astype(np.float64).tolist(), used["cls_conf"].astype(np.float64).tolist()
        # per-image mean classifier confidence in one pass (a NumPy slice + mean per image cost 5 us each): float64 sums of the
        # float32 probabilities, as the reference's np.mean over Python floats (e2e.py:500-501)
        img_of = np.repeat(np.arange(B), cnt_a)
        ok = used["cls_class"] >= 0
        n_ok = np.bincount(img_of, weights=ok, minlength=B)
        s_ok = np.bincount(img_of, weights=np.where(ok, used["cls_conf"].astype(np.float64), 0.0), minlength=B)
        cls_avg = (s_ok / np.maximum(n_ok, 1.0)).tolist()
        n_ok = n_ok.tolist()
        num_det_l = np.asarray(num_det[:B]).tolist()
        conf_avg_l = np.asarray(conf_avg[:B], dtype=np.float64).tolist()
        t_det, t_roi, t_cls, t_tot = timing.t_detection / B, timing.t_roi_extract / B, timing.t_classification / B, wall_ms / B
        fps = 1000.0 / t_tot if t_tot > 0 else 0
        cpu_p, mem_mb, temp = sysm
        if topk is not None:   # the valid entries of every used record, [(class, prob), ...]
            ku = topk[:B][np.arange(topk.shape[1])[None, :] < cnt_a[:, None]]
            topk_cols = [[(c, p) for c, p in zip(cs, ps) if c >= 0] for cs, ps in zip(ku["cls"].tolist(), ku["prob"].astype(np.float64).tolist())]
        if quality is not None:   # every used record's four figures; None for a detection without a crop
            qu = quality[:B][np.arange(quality.shape[1])[None, :] < cnt_a[:, None]]
            ok = (qu["flags"] & _ffi.LP_QUALITY_VALID) != 0
            qual_cols = [dict(zip(QUALITY_RESULT_KEYS, v)) if o else dict.fromkeys(QUALITY_RESULT_KEYS)
                         for o, v in zip(ok.tolist(), zip(*(qu[k].astype(np.float64).tolist() for k in QUALITY_RESULT_KEYS)))]
        if tracks is not None:
            tu = tracks[:B][np.arange(tracks.shape[1])[None, :] < cnt_a[:, None]]
            trk_cols = list(zip(tu["track_id"].tolist(), tu["hits"].tolist(), tu["age"].tolist(), tu["voted_class"].tolist(),
                                tu["voted_conf"].astype(np.float64).tolist(), ((tu["flags"] & _ffi.LP_TRACK_CONFIRMED) != 0).tolist()))
        out = []
        pos = 0
        for i in range(B):
            # device stage times are per batch call; report the per-image share like a sequential loop would
            nd = num_det_l[i]   # counted BEFORE the min-area filter (e2e.py:454)
            n = cnt[i]
            # det_confidence_avg: averaged over ALL detector boxes, before the min-area filter (e2e.py:456-457)
            m = PipelineMetrics(t_detection=t_det, t_roi_extract=t_roi, t_classification=t_cls, t_total=t_tot, fps=fps, num_detections=nd,
                                det_confidence_avg=conf_avg_l[i] if nd else 0.0, cls_confidence_avg=cls_avg[i] if n_ok[i] else 0.0,
                                cpu_percent=cpu_p, memory_mb=mem_mb, temperature=temp)
            results = []
            if n:
                td, tc = t_det / n, t_cls / n
                e = pos + n
                results = [{"bbox": bb, "det_class": dc, "det_conf": df, "cls_class": cc, "cls_conf": cf, "time_det": td, "time_cls": tc}
                           for bb, dc, df, cc, cf in zip(boxes[pos:e], det_cls[pos:e], det_cf[pos:e], cls_cls[pos:e], cls_cf[pos:e])]
                if topk is not None:
                    for r, tk in zip(results, topk_cols[pos:e]):
                        r["cls_topk"] = tk
                if quality is not None:
                    for r, qd in zip(results, qual_cols[pos:e]):
                        r.update(qd)
                if tracks is not None:
                    for r, (tid, th, ta, tc_, tcc, tok) in zip(results, trk_cols[pos:e]):
                        r.update(track_id=tid, track_hits=th, track_age=ta, track_cls=tc_, track_cls_conf=tcc, track_confirmed=tok)
                pos = e
            out.append((results, m))
        return out

    def run(self, image: np.ndarray, conf_threshold: float = 0.5, iou_threshold: float = 0.45,
            min_area: int = 100) -> Tuple[List[Dict], PipelineMetrics]:
        return self.run_batch([image], conf_threshold, iou_threshold, min_area, **({"evaluate": False} if self.evaluate else {}))[0]

    def evaluation(self, reset: bool = False) -> Dict:
        """The metrics of everything run_batch(gts=...) fed the evaluator (synchronises): evaluate_predictions' dict, from the
        drained rows (litepi.e2e.metrics_from_rows); eval_frames and eval_rows_dropped then hold the frames scored and the rows
        lost to a full log.  reset: empty the evaluator afterwards."""
        if not self.evaluate:
            raise ValueError("evaluation needs a pipeline constructed with evaluate=True or an evaluator configuration")
        from .e2e import metrics_from_rows
        got = self.engine.eval_drain()
        m = metrics_from_rows(got["rows"], got["gt_per_class"], self.engine.cfg.num_classes, self.engine.eval_cfg.n_thr)
        self.eval_frames, self.eval_rows_dropped = got["frames"], got["dropped"]
        if reset:
            self.engine.eval_reset()
        return m
