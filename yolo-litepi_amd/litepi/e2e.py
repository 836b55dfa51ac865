#!/usr/bin/env python3
"""End-to-end evaluation CLI with the argument surface of the reference's
``src/tt100k/pipeline/e2e.py`` (flags and defaults: e2e.py:1017-1048), running on the HIP
backend.  Same two passes per image (benchmark pass at ``--benchmark_conf`` whose time feeds the
FPS figure, evaluation pass at ``--yolo_conf`` that feeds mAP; e2e.py:955-1011), same
Ultralytics-style metric (e2e.py:656-824) and the same appended ``comparison_summary.csv`` schema
(e2e.py:1166-1184).  New flags: ``--batch_images``, ``--precision``, ``--hip_device``, ``--gpus``.

``--raw_frames FILE --frame_size WxH --pixel_format nv12|bgr [--csc_matrix bt601|bt709]``: the frames come from a headerless
file of concatenated frames (what ``ffmpeg -pix_fmt nv12 -f rawvideo`` writes) instead of the images under ``--input``; they
are named ``frame_000001`` ..., go through the same batching, sharding, result rows and CSV, and a frame's ground truth is
``<name>.txt`` under ``--labels``.  NV12 frames are converted on the device.

``--gpus N`` (launched as ``python -m torch.distributed.run --nproc-per-node N -m litepi.e2e ... --gpus N``): one process
per GPU, the sorted image list is sharded contiguously (``distributed.shard_range``), every rank runs both passes on its
shard with a full weight replica, the per-image predictions and ground truths are gathered to rank 0 once
(``distributed.gather_eval_shards``, backend nccl = RCCL), and rank 0 alone scores, prints and writes the CSV.  The FPS
figure of a multi-rank run is images / the slowest rank's summed benchmark time (the wall time of the sharded job).

Differences, on purpose: images are decoded with Pillow (cv2 is not a dependency);
``--detector_threads`` and ``--device`` are accepted and ignored (everything runs on the GPU);
all four ``--clf_arch`` choices run on the GPU; ``--save_viz`` overlays (e2e.py:826-884, 1003-1009) are drawn with Pillow: same
layout and colours as the reference's cv2 drawing (ground truth blue, predictions green, label boxes, summary bar), Pillow's
default font instead of Hershey.
"""
from __future__ import annotations

import argparse
import json
import os
import random
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


# ------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="E2E HIP (MI355X) detector + classifier evaluation pipeline")
    p.add_argument("--detector_param", type=str, default="../convert/model/yolo_plus/yolo_plus_ncnn_model/model.ncnn.param")
    p.add_argument("--detector_bin", type=str, default="../convert/model/yolo_plus/yolo_plus_ncnn_model/model.ncnn.bin")
    p.add_argument("--detector_onnx", type=str, default=None,
                   help="an ONNX export of the detector; overrides --detector_param / --detector_bin")
    p.add_argument("--classifier", type=str, default="../weight/shufflenetv2.pth")
    p.add_argument("--clf_arch", type=str, choices=["resnet18", "efficientnet", "mobilenetv2", "shufflenetv2"], default="shufflenetv2")
    p.add_argument("--input", type=str, default="../Dataset/E2E/data_e2e_tt100k/images/test")
    p.add_argument("--labels", type=str, default="../Dataset/E2E/data_e2e_tt100k/labels/test")
    p.add_argument("--classes", type=str, default="../Dataset/E2E/data_e2e_tt100k/idx2label.json")
    p.add_argument("--num_samples", type=int, default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--yolo_conf", type=float, default=0.001)
    p.add_argument("--benchmark_conf", type=float, default=0.25)
    p.add_argument("--min_area", type=int, default=50)
    p.add_argument("--iou_threshold", type=float, default=0.45)
    p.add_argument("--det_input_size", type=det_input_size_arg, default=640,
                   help="detector input: an integer (square) or ROWSxCOLUMNS, e.g. 384x640 for 16:9 video; both multiples of 32")
    p.add_argument("--cls_input_size", type=int, default=64)
    p.add_argument("--detector_threads", type=int, default=4, help="ignored (NCNN threads in the reference)")
    p.add_argument("--batch_size", type=int, default=8, help="kept for compatibility: all ROIs of a call are classified together")
    p.add_argument("--device", type=str, choices=["cpu", "cuda", "hip"], default="hip", help="ignored: always the HIP device")
    p.add_argument("--output", type=str, default="output_eval")
    p.add_argument("--save_viz", default=False, help="write visualizations/vis_<image>.png overlays like the reference (any non-empty value)")
    # new
    p.add_argument("--batch_images", type=int, default=1, help="images per GPU call")
    p.add_argument("--precision", type=str, choices=["fp16", "fp32"], default="fp16")
    p.add_argument("--hip_device", type=int, default=0)
    p.add_argument("--gpus", type=int, default=1,
                   help="GPUs of this node to shard the image list over: one process per GPU under torch.distributed.run "
                        "(WORLD_SIZE must equal --gpus; the rank's GPU is LOCAL_RANK and overrides --hip_device)")
    p.add_argument("--max_det", type=int, default=0,
                   help="detections kept per image; 0 = one slot per anchor, i.e. nothing is ever dropped (what the reference does: "
                        "e2e.py:280-296 keeps every NMS survivor, and the evaluation pass at --yolo_conf 0.001 produces thousands)")
    p.add_argument("--max_rois", type=int, default=0, help="classifier capacity per call; 0 = batch_images x max_det")
    p.add_argument("--numerics", type=str, choices=["e2e", "e2e_optimize"], default="e2e",
                   help="which reference pipeline's ROI stage to follow: e2e.py (PIL antialiased resize) or e2e_optimize.py "
                        "(cv2-linear resize, its own clip rule)")
    # e2e_optimize.py's extras (e2e_optimize.py:882-885)
    p.add_argument("--warmup", type=int, default=None,
                   help="warm-up passes on a random 640x640 frame before the timed loop (e2e_optimize.py:552-570 warmup_pipeline); "
                        "default 10 under --numerics e2e_optimize as there, 0 otherwise (e2e.py has none).  Here they also take "
                        "the hipGraph capture of the benchmark pass out of the first timed image")
    p.add_argument("--tile_overlap", type=int, default=None,
                   help="tiled inference (off when absent): frames larger than det_input are also seen as native-resolution "
                        "det_input crops overlapping by this many pixels, merged by one NMS per frame; the handle holds "
                        "batch_images x the views of a 2048x2048 frame")
    p.add_argument("--tile_full_frame", type=int, choices=[0, 1], default=1,
                   help="tiled inference: the letterboxed whole frame is an extra view of every frame that needs crops")
    p.add_argument("--view_tile", type=int, default=None,
                   help="scaled views (off when absent): every frame is also seen through windows of this many pixels, each "
                        "letterboxed to det_input (a 1280 window at det_input 640 is a half-resolution look), overlapping by "
                        "--view_overlap, merged by one NMS per frame; excludes --tile_overlap and --views")
    p.add_argument("--view_overlap", type=int, default=0, help="scaled views: pixels shared by neighbouring --view_tile windows")
    p.add_argument("--view_full_frame", type=int, choices=[0, 1], default=1,
                   help="scaled views: the letterboxed whole frame is an extra view of every frame that needs more than one window")
    p.add_argument("--views", type=str, default=None,
                   help='scaled views given one by one, applied to every frame: "full;x,y,w,h;..." (full = the letterboxed whole '
                        'frame; x,y,w,h = a source window in frame pixels, letterboxed to det_input at its own scale)')
    p.add_argument("--view_maps", type=str, default=None,
                   help="mapped views (off when absent): an .npz with xy [M, S, S, 2] float32 remap tables (S = --det_input_size; "
                        "frame positions of every view pixel, cv2.remap's convention; litepi.lens builds them) and frame [2] = "
                        "(H, W) of the frames they belong to; every frame is seen through --views (if given) and through every "
                        "map, merged by one NMS per frame; excludes --tile_overlap, --view_tile and --focus")
    p.add_argument("--focus", type=int, default=None,
                   help="focus views (off when absent; needs --track): every frame is seen through the whole frame and this many "
                        "windows the tracker chooses on the device -- native-resolution looks at the small tracked signs, the free "
                        "ones swept over the frame -- and focus.csv lists the windows of every frame; excludes --tile_overlap, "
                        "--view_tile and --views")
    p.add_argument("--focus_side_max", type=int, default=0, help="focus views: the largest window side (0 = 2 x det_input)")
    p.add_argument("--focus_margin", type=float, default=2.0, help="focus views: a window's side is this many times the box's longer side")
    p.add_argument("--no_focus_sweep", action="store_true", help="focus views: leave the free window slots empty instead of sweeping the frame")
    p.add_argument("--view_match", type=str, choices=["iou", "ios"], default=None,
                   help="how the boxes of one frame's views are matched (needs --tile_overlap, --view_tile, --views or --focus): iou = the "
                        "reference's rule; ios = intersection over the smaller box, which pairs a sign cut by a view border with the whole one")
    p.add_argument("--view_merge", type=str, choices=["nms", "union"], default=None,
                   help="what a match does: nms = the lower box is dropped; union = the kept box grows to cover what it absorbed")
    p.add_argument("--view_match_thr", type=float, default=None, help="threshold of --view_match (absent or 0: --iou_threshold)")
    p.add_argument("--raw_frames", type=str, default=None,
                   help="headerless file of concatenated video frames (ffmpeg -f rawvideo) evaluated instead of the images of --input; "
                        "needs --frame_size; frames are named frame_000001, frame_000002, ...")
    p.add_argument("--frame_size", type=str, default=None, help="WxH of the frames of --raw_frames, e.g. 1280x720")
    p.add_argument("--pixel_format", type=str, choices=["bgr", "nv12"], default="bgr",
                   help="pixel format of the frames of --raw_frames: packed bgr24, or nv12 (converted on the device)")
    p.add_argument("--csc_matrix", type=str, choices=["bt601", "bt709"], default="bt601",
                   help="YCbCr matrix of nv12 frames (limited range): bt601 = cv2's COLOR_YUV2BGR_NV12, bt709 = HD video")
    p.add_argument("--track", action="store_true",
                   help="track the signs across the frames of --raw_frames (a sequence) on the device and write tracks.csv: identity, "
                        "voted class, hits and confirmation per detection of the benchmark pass")
    p.add_argument("--inventory", action="store_true",
                   help="with --track: one row per finished track in signs.csv (final voted class, first / last frame, best sighting) "
                        "and the classifier's input crop of the best sighting as signs/sign_<stream>_<track>.png; collected on the device")
    p.add_argument("--inventory_best", choices=["area", "det_conf", "cls_conf", "sharpness"], default="area",
                   help="what makes a sighting the best of its track; sharpness: the variance of the Laplacian of its classifier crop "
                        "(implies --quality)")
    p.add_argument("--quality", action="store_true",
                   help="with --track: measure sharpness and exposure of every detection's classifier crop on the device; tracks.csv "
                        "gains the columns sharpness, luma_mean, clip_lo, clip_hi at the end (empty for a detection without a crop)")
    p.add_argument("--inventory_evidence", type=int, default=None, metavar="E",
                   help="with --track --inventory: also keep an E x E BGR picture of the surroundings of every sign's best sighting "
                        "(a multiple of 16 in 32..256), written as signs/sign_<stream>_<track>_evidence.png; signs.csv gains the "
                        "picture's window in the frame")
    p.add_argument("--inventory_evidence_scale", type=float, default=None, metavar="S",
                   help="side of the picture's window as a multiple of the box's longer side, 1..16 (default 2)")
    p.add_argument("--track_iou", type=float, default=0.3, help="a detection matches a track when their IoU exceeds this")
    p.add_argument("--track_max_age", type=int, default=5, help="frames a track may stay unmatched before it is dropped")
    p.add_argument("--track_min_hits", type=int, default=3, help="matched frames after which a track counts as confirmed")
    p.add_argument("--topk", type=int, default=None, metavar="K",
                   help="off when absent: every result also carries the K (1..8) most probable classes of the classifier's "
                        "distribution with their probabilities (cls_topk); the CSV files and the overlays stay as they are")
    p.add_argument("--track_vote", type=str, choices=["top1", "distribution"], default="top1",
                   help="with --track: what a detection adds to its track's class vote -- top1: its arg-max class and confidence; "
                        "distribution: its K most probable classes, each with its probability (needs --topk K)")
    p.add_argument("--device_eval", action="store_true",
                   help="score the evaluation pass on the device: every chunk's parsed labels go to run_batch(gts=...) and the metrics "
                        "come from the engine's evaluator (lp_eval_*) instead of evaluate_predictions; CSVs and overlays are as before.  "
                        "This command reads image files and gains no time from it: the gain is for callers whose frames and "
                        "detections stay on the device.  Not with --gpus N > 1")
    p.add_argument("--device_eval_max_gt", type=int, default=64, help="with --device_eval: the most boxes a label file may hold (1..256)")
    p.add_argument("--no_jit", action="store_true", help="accepted and ignored: there is no TorchScript on this path (e2e_optimize.py:884)")
    return p


def det_input_size_arg(text):
    """--det_input_size: "640" -> 640, "384x640" -> (384, 640) (rows x columns)."""
    t = str(text).strip().lower()
    try:
        if "x" in t:
            rows, cols = t.split("x")
            return int(rows), int(cols)
        return int(t)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--det_input_size takes an integer or ROWSxCOLUMNS, got {text!r}") from None


def num_anchors(det_input_size) -> int:
    """Anchor points of the Detect head on a square input: one per cell of the stride-8/16/32 grids (8400 at 640)."""
    h, w = (det_input_size if isinstance(det_input_size, (tuple, list)) else (det_input_size, det_input_size))
    return sum(((int(h) + s - 1) // s) * ((int(w) + s - 1) // s) for s in (8, 16, 32))


def load_class_names(path: str) -> List[str]:
    """JSON {"idx": "name"} or one name per line (e2e.py:160-176)."""
    with open(path, "r") as f:
        text = f.read()
    try:
        data = json.loads(text)
    except json.JSONDecodeError:
        return [ln.strip() for ln in text.splitlines() if ln.strip()]
    if not isinstance(data, dict):
        raise ValueError("JSON must be a dictionary")
    names = [""] * (max(int(k) for k in data) + 1)
    for k, v in data.items():
        names[int(k)] = v
    return names


def parse_yolo_label(label_path, img_w: int, img_h: int) -> List[Tuple[int, int, int, int, int]]:
    """``cls xc yc w h`` normalised -> (cls, x1, y1, x2, y2) int pixels (e2e.py:137-157)."""
    if not os.path.exists(label_path):
        return []
    out = []
    with open(label_path) as f:
        for line in f:
            t = line.split()
            if len(t) < 5:
                continue
            xc, yc, w, h = (float(v) for v in t[1:5])
            out.append((int(t[0]), int((xc - w / 2) * img_w), int((yc - h / 2) * img_h), int((xc + w / 2) * img_w),
                        int((yc + h / 2) * img_h)))
    return out


def sample_images(files: Sequence, num_samples: Optional[int], seed: int = 42):
    """Deterministic subset (e2e.py:179-186)."""
    if num_samples is None or num_samples <= 0 or num_samples >= len(files):
        return list(files)
    random.seed(seed)
    return sorted(random.sample(list(files), num_samples))


def visualize_prediction(img_bgr: np.ndarray, predictions: Sequence[Dict], ground_truths, class_names: Sequence[str], output_path) -> None:
    """Ground truths (blue) and predictions (green) drawn on the image, like the reference's visualize_prediction
    (e2e.py:826-884): 3-px rectangles, "GT: <name>" above each ground truth, "PRED: <name>" and "Cls:x Det:y" below each
    prediction on filled label boxes, and the "GT: n | Predictions: m" bar in the top-left corner.  Drawn with Pillow (RGB)."""
    from PIL import Image, ImageDraw, ImageFont
    im = Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1]))
    d = ImageDraw.Draw(im)
    font = ImageFont.load_default()
    h, w = img_bgr.shape[:2]
    BLUE, GREEN, DGREEN, WHITE, BLACK = (0, 0, 255), (0, 255, 0), (0, 200, 0), (255, 255, 255), (0, 0, 0)

    def name_of(i):
        return class_names[i] if 0 <= int(i) < len(class_names) else str(i)

    def label(x, y_base, text, fill):
        l, t, r, b = d.textbbox((0, 0), text, font=font)
        tw, th = r - l, b - t
        d.rectangle([x, y_base - th - 4, x + tw + 2, y_base + 2], fill=fill)
        d.text((x + 1, y_base - th - 2), text, fill=WHITE, font=font)
        return th

    for gt_cls, x1, y1, x2, y2 in ground_truths:
        d.rectangle([x1, y1, x2, y2], outline=BLUE, width=3)
        label(x1, max(y1 - 10, 15), f"GT: {name_of(gt_cls)}", BLUE)
    for pred in predictions:
        x1, y1, x2, y2 = [int(v) for v in pred["bbox"]]
        d.rectangle([x1, y1, x2, y2], outline=GREEN, width=3)
        ty = min(y2 + 25, h - 5)
        th = label(x1, ty, f"PRED: {name_of(pred['cls_class'])}", GREEN)
        label(x1, ty + th + 7, f"Cls:{pred['cls_conf']:.2f} Det:{pred['det_conf']:.2f}", DGREEN)
    d.rectangle([5, 5, 400, 35], fill=BLACK)
    d.text((10, 14), f"GT: {len(ground_truths)} | Predictions: {len(predictions)}", fill=WHITE, font=font)
    im.save(str(output_path))


class RawFrame:
    """One frame of a --raw_frames file, standing where an image path stands in the evaluation loop."""

    def __init__(self, index: int, parent: Path):
        self.index, self.parent = index, parent
        self.name = self.stem = f"frame_{index + 1:06d}"

    def __lt__(self, other):
        return self.index < other.index


def parse_frame_size(text: Optional[str]) -> Tuple[int, int]:
    """"WxH" -> (W, H)."""
    try:
        w, h = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise ValueError(f"--frame_size must be WxH, e.g. 1280x720 (got {text!r})") from None
    if w <= 0 or h <= 0:
        raise ValueError(f"--frame_size must be positive (got {text!r})")
    return w, h


def read_raw_frames(path, width: int, height: int, pixel_format: str = "nv12") -> np.ndarray:
    """The frames of a headerless file of concatenated frames as one read-only array: [n, H * 3 // 2, W] for nv12 (the
    host frame shape of the backend), [n, H, W, 3] for bgr.  A trailing partial frame is an error."""
    if pixel_format == "nv12":
        if width % 2 or height % 2:
            raise ValueError(f"NV12 frames need an even width and height (got {width}x{height})")
        shape = (height * 3 // 2, width)
    elif pixel_format == "bgr":
        shape = (height, width, 3)
    else:
        raise ValueError(f"unknown pixel format {pixel_format!r}")
    nbytes = int(np.prod(shape))
    size = os.path.getsize(path)
    if size == 0 or size % nbytes:
        raise ValueError(f"{path}: {size} bytes is not a whole number of {width}x{height} {pixel_format} frames of {nbytes} bytes "
                         f"({size // nbytes} frames and {size % nbytes} bytes left over)")
    return np.memmap(path, dtype=np.uint8, mode="r", shape=(size // nbytes,) + shape)


def read_image_bgr(path) -> Optional[np.ndarray]:
    from PIL import Image
    try:
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
    except Exception:  # noqa: BLE001 - unreadable image -> skipped, like cv2.imread returning None
        return None


# ------------------------------------------------------------------------------------------------
def _pairwise_iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[:, :2])
    rb = np.minimum(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clip(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b - inter + 1e-7)


def _ap101(recall: np.ndarray, precision: np.ndarray) -> float:
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return float(trapz(np.interp(x, mrec, mpre), x))


def match_predictions(all_preds, all_gts, iou_thresholds=np.arange(0.5, 1.0, 0.05)) -> List:
    """The per-frame matching of evaluate_predictions: one (correct [P, n_thr] bool, conf [P], cls [P], ground-truth classes)
    per frame that holds a prediction or a ground truth.  Per IoU threshold, matches are ranked by IoU and de-duplicated per
    prediction, then per ground truth; a match counts only when the CLASSIFIER class equals the label."""
    nt = len(iou_thresholds)
    stats = []
    for preds, gts in zip(all_preds, all_gts):
        if len(preds) == 0:
            if len(gts) > 0:
                stats.append((np.zeros((0, nt), bool), np.array([]), np.array([]), np.array(gts)[:, 0]))
            continue
        pb = np.array([p["bbox"] for p in preds])
        pconf = np.array([p["conf"] for p in preds])
        pcls = np.array([p["cls_class"] for p in preds])
        correct = np.zeros((len(preds), nt), bool)
        if len(gts) > 0:
            g = np.array(gts)
            tcls, tb = g[:, 0], g[:, 1:]
            iou = _pairwise_iou(pb, tb)
            for j, thr in enumerate(iou_thresholds):
                pi, gi = np.where(iou >= thr)
                if not len(pi):
                    continue
                m = np.concatenate((np.stack((pi, gi), 1), iou[pi, gi][:, None]), 1)
                if len(pi) > 1:
                    m = m[m[:, 2].argsort()[::-1]]
                    m = m[np.unique(m[:, 0], return_index=True)[1]]
                    m = m[np.unique(m[:, 1], return_index=True)[1]]
                for p_i, g_i, _ in m:
                    if pcls[int(p_i)] == tcls[int(g_i)]:
                        correct[int(p_i), j] = True
        else:
            tcls = np.array([])
        stats.append((correct, pconf, pcls, tcls))
    return stats


def evaluate_predictions(all_preds, all_gts, num_classes, iou_threshold=0.5, iou_thresholds=np.arange(0.5, 1.0, 0.05)) -> Dict:
    """Ultralytics-style global evaluation with the semantics of the reference (e2e.py:656-824):
    per IoU threshold, matches are ranked by IoU, de-duplicated per prediction then per ground
    truth, and count only when the CLASSIFIER class equals the label; predictions are ranked
    globally by detector confidence; AP is the 101-point interpolated area; the means run over the
    classes present in the ground truth.  ``iou_threshold`` is unused, as in the reference.  The matching is
    match_predictions, the ranking and the AP integral evaluate_from_rows."""
    stats = match_predictions(all_preds, all_gts, iou_thresholds)
    if not stats:
        return _empty_metrics(num_classes)
    tp = np.concatenate([s[0] for s in stats], 0)
    conf = np.concatenate([s[1] for s in stats], 0)
    pcls = np.concatenate([s[2] for s in stats], 0)
    tcls = np.concatenate([s[3] for s in stats], 0)
    uniq, counts = np.unique(tcls, return_counts=True)
    return _metrics_tail(tp, conf, pcls, uniq, counts, num_classes)


def _empty_metrics(num_classes) -> Dict:
    zeros = lambda: np.zeros(num_classes)  # noqa: E731
    return {"precision": zeros(), "recall": zeros(), "f1": zeros(), "tp": zeros(), "fp": zeros(), "fn": zeros(),
            "mAP50": 0.0, "mAP50_95": 0.0, "classes_present": np.zeros(num_classes, dtype=bool)}


def evaluate_from_rows(tp, conf, pcls, gt_per_class, num_classes) -> Dict:
    """The tail of evaluate_predictions: tp [N, n_thr] bool, conf [N] float64 and pcls [N], one row per prediction in frame
    order, and gt_per_class [num_classes], the ground-truth boxes per class.  Ranks the rows globally by confidence and
    integrates AP per class; the dict evaluate_predictions returns."""
    gt_per_class = np.asarray(gt_per_class, dtype=np.int64)
    if len(conf) == 0 and not gt_per_class.any():   # no frame held a prediction or a ground truth
        return _empty_metrics(num_classes)
    uniq = np.flatnonzero(gt_per_class)   # what np.unique(tcls, return_counts=True) gives for classes inside 0..num_classes-1
    return _metrics_tail(tp, conf, pcls, uniq, gt_per_class[uniq], num_classes)


def _metrics_tail(tp, conf, pcls, uniq, counts, num_classes) -> Dict:
    """everything of evaluate_predictions from the global ranking on; uniq / counts: the ground-truth classes present and
    their numbers of boxes, as np.unique(tcls, return_counts=True) returns them"""
    zeros = lambda: np.zeros(num_classes)  # noqa: E731
    order = np.argsort(-conf)
    tp, pcls = tp[order], pcls[order]
    n_gt_of = dict(zip(uniq, counts))
    ap50, ap5095, pbest, rbest, fbest = zeros(), zeros(), zeros(), zeros(), zeros()
    tpc_, fpc_, fnc_ = zeros(), zeros(), zeros()
    for c in range(num_classes):
        n_gt = n_gt_of.get(c, 0)
        sel = pcls == c
        n_p = sel.sum()
        if n_p == 0 and n_gt == 0:
            continue
        if n_p == 0 or n_gt == 0:
            fnc_[c] = n_gt
            continue
        tpc = tp[sel].cumsum(0)
        fpc = (1 - tp[sel]).cumsum(0)
        rec = tpc / (n_gt + 1e-16)
        prec = tpc / (tpc + fpc + 1e-16)
        aps = [_ap101(rec[:, j], prec[:, j]) for j in range(tp.shape[1])]
        ap50[c], ap5095[c] = aps[0], np.mean(aps)
        f1 = 2 * prec[:, 0] * rec[:, 0] / (prec[:, 0] + rec[:, 0] + 1e-16)
        b = int(np.argmax(f1))
        pbest[c], rbest[c], fbest[c] = prec[b, 0], rec[b, 0], f1[b]
        tpc_[c], fpc_[c] = tpc[b, 0], fpc[b, 0]
        fnc_[c] = n_gt - tpc_[c]
    present = uniq.astype(int)
    return {"precision": pbest, "recall": rbest, "f1": fbest, "tp": tpc_, "fp": fpc_, "fn": fnc_,
            "mAP50": float(np.mean(ap50[present])) if len(present) else 0.0,
            "mAP50_95": float(np.mean(ap5095[present])) if len(present) else 0.0,
            "ap50_per_class": ap50, "classes_present": np.isin(np.arange(num_classes), uniq)}


def metrics_from_rows(rows, gt_per_class, num_classes, n_thr) -> Dict:
    """The metrics of an evaluator's drained log (Engine.eval_drain): rows are EVAL_ROW_DTYPE records in frame order, then
    record order.  Bit j of `correct` becomes column j of the boolean matrix, conf the float64 of the float32 det_conf, as
    the result dicts carry it, and the same tail as evaluate_predictions does the rest: the same arrays into the same numpy
    calls, so also the same order among equal confidences."""
    rows = np.asarray(rows)
    tp = ((rows["correct"][:, None] >> np.arange(n_thr, dtype=np.uint32)[None, :]) & 1).astype(bool)
    return evaluate_from_rows(tp, rows["conf"].astype(np.float64), rows["cls"].astype(np.int64), gt_per_class, num_classes)


# ------------------------------------------------------------------------------------------------
TRACKS_CSV_COLUMNS = ("frame", "track_id", "x1", "y1", "x2", "y2", "det_conf", "cls_class", "cls_conf", "voted_class", "voted_conf", "hits",
                      "confirmed")


SIGNS_CSV_COLUMNS = ("stream", "track_id", "first_frame", "last_frame", "hits", "voted_class", "voted_conf", "best_frame", "x1", "y1", "x2",
                     "y2", "det_class", "flushed", "crop")
QUALITY_CSV_COLUMNS = ("sharpness", "luma_mean", "clip_lo", "clip_hi")   # --quality: appended to tracks.csv, at the end
EVIDENCE_CSV_COLUMNS = ("evidence_x", "evidence_y", "evidence_w", "evidence_h")   # --inventory_evidence: the picture's window, at the end


def quality_wanted(args) -> bool:
    """--quality, or implied by --inventory_best sharpness"""
    return bool(getattr(args, "quality", False)) or getattr(args, "inventory_best", "area") == "sharpness"


def parse_views(text: str) -> List:
    """--views "full;x,y,w,h;..." -> ["full", (x, y, w, h), ...]"""
    out = []
    for part in text.split(";"):
        part = part.strip()
        if part == "full":
            out.append("full")
            continue
        try:
            x, y, w, h = (int(v) for v in part.split(","))
        except ValueError:
            raise SystemExit(f'--views: {part!r} is neither "full" nor x,y,w,h') from None
        out.append((x, y, w, h))
    if not out:
        raise SystemExit("--views needs at least one view")
    return out


def load_view_maps(path: str, det_input_size):
    """--view_maps FILE.npz -> (xy [M, S, S, 2] float32, (H, W))"""
    size = det_input_size if isinstance(det_input_size, tuple) else (det_input_size, det_input_size)
    try:
        with np.load(path) as z:
            if "xy" not in z.files or "frame" not in z.files:
                raise SystemExit(f"--view_maps {path}: the file holds {sorted(z.files)}, it needs xy [M, S, S, 2] and frame [2]")
            xy, frame = np.asarray(z["xy"]), np.asarray(z["frame"]).reshape(-1)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--view_maps {path}: {e}") from None
    if xy.ndim != 4 or xy.shape[0] < 1 or xy.shape[1] != xy.shape[2] or xy.shape[3] != 2 or xy.shape[1] != size[1]:
        raise SystemExit(f"--view_maps {path}: xy is {xy.shape}, it needs [M, {size[1]}, {size[1]}, 2] for --det_input_size {size[1]}")
    if len(frame) != 2 or min(int(v) for v in frame) < 1:
        raise SystemExit(f"--view_maps {path}: frame is {frame.tolist()}, it needs (H, W)")
    if np.isnan(xy).any():
        raise SystemExit(f"--view_maps {path}: xy holds a NaN")
    return np.ascontiguousarray(xy, dtype=np.float32), (int(frame[0]), int(frame[1]))


def list_inputs(args):
    """What a run processes: (files, raw, label_dir, (fw, fh)) -- the frames of --raw_frames (raw: the memory-mapped file), the
    one image --input names, or the images of the --input directory, sampled by --num_samples."""
    inp = Path(args.input)
    raw, fw, fh = None, 0, 0
    if args.raw_frames:
        fw, fh = parse_frame_size(args.frame_size)
        raw = read_raw_frames(args.raw_frames, fw, fh, args.pixel_format)
        label_dir = Path(args.labels) if args.labels else None
        files = [RawFrame(i, Path(args.raw_frames).parent) for i in range(len(raw))]
        if args.num_samples:
            files = sample_images(files, args.num_samples, args.seed)
    elif inp.is_file():
        files = [inp]
        label_dir = Path(args.labels) if args.labels else None
    else:
        label_dir = Path(args.labels) if args.labels else inp / "labels"
        files = sorted(list(inp.glob("*.jpg")) + list(inp.glob("*.png")) + list(inp.glob("*.jpeg")))
        if args.num_samples:
            files = sample_images(files, args.num_samples, args.seed)
    return files, raw, label_dir, (fw, fh)


def check_device_eval_labels(gts, max_gt: int, name) -> None:
    """--device_eval: a label file with more boxes than the evaluator holds per frame is refused"""
    if len(gts) > max_gt:
        raise SystemExit(f"--device_eval: {name} holds {len(gts)} boxes, more than --device_eval_max_gt {max_gt}")


def check_frame_args(args) -> None:
    if getattr(args, "device_eval", False):
        if args.gpus > 1:
            raise SystemExit(f"--device_eval and --gpus {args.gpus} exclude each other: the sharded gather of the evaluator's rows is "
                             f"not supported")
        if not 1 <= getattr(args, "device_eval_max_gt", 64) <= 256:
            raise SystemExit(f"--device_eval_max_gt {args.device_eval_max_gt} outside 1..256")
    modes = [n for n in ("tile_overlap", "view_tile", "views", "focus") if getattr(args, n, None) is not None]
    if len(modes) > 1:
        raise SystemExit("--" + ", --".join(modes) + " exclude each other: one way of looking at a frame per run")
    if getattr(args, "view_maps", None) is not None:
        clash = [n for n in modes if n != "views"]
        if clash:
            raise SystemExit(f"--view_maps and --{clash[0]} exclude each other: maps combine with --views only")
        modes = modes + ["view_maps"]
    merge_set = [n for n in ("view_match", "view_merge", "view_match_thr") if getattr(args, n, None) is not None]
    if merge_set and not modes:
        raise SystemExit("--" + ", --".join(merge_set) + " need one of --tile_overlap, --view_tile, --views or --focus: a frame seen "
                         "through one letterboxed view has nothing to merge")
    thr = getattr(args, "view_match_thr", None)
    if thr is not None and not 0.0 <= thr < 1.0:
        raise SystemExit(f"--view_match_thr {thr} outside [0, 1)")
    size = getattr(args, "det_input_size", 640)
    if modes and isinstance(size, tuple) and size[0] != size[1]:
        raise SystemExit(f"--{modes[0]} needs a square --det_input_size (it is {size[0]}x{size[1]}): frame views on a rectangular "
                         f"detector input are not supported")
    if getattr(args, "views", None) is not None:
        parse_views(args.views)
    if getattr(args, "view_maps", None) is not None:
        load_view_maps(args.view_maps, size)
    if getattr(args, "focus", None) is not None:
        if not getattr(args, "track", False):
            raise SystemExit("--focus needs --track: the windows are chosen from the tracker's state")
        if not 1 <= args.focus <= 16:
            raise SystemExit(f"--focus {args.focus} outside 1..16 window slots")
    topk, vote = getattr(args, "topk", None), getattr(args, "track_vote", "top1")
    if topk is not None and not 1 <= topk <= 8:
        raise SystemExit(f"--topk {topk} outside 1..8 classes per detection")
    if vote == "distribution" and not (getattr(args, "track", False) and topk is not None):
        raise SystemExit("--track_vote distribution needs --track and --topk K: the tracker then votes with every detection's "
                         "K most probable classes")
    if getattr(args, "inventory", False) and not getattr(args, "track", False):
        raise SystemExit("--inventory needs --track: the inventory lists the tracker's finished tracks")
    if getattr(args, "inventory_best", "area") == "sharpness" and not (getattr(args, "track", False) and getattr(args, "inventory", False)):
        raise SystemExit("--inventory_best sharpness needs --track --inventory: it ranks the sightings of the inventory's tracks")
    if getattr(args, "quality", False) and not getattr(args, "track", False):
        raise SystemExit("--quality needs --track: the figures are written to tracks.csv")
    if getattr(args, "inventory_evidence", None) is not None or getattr(args, "inventory_evidence_scale", None) is not None:
        if not (getattr(args, "track", False) and getattr(args, "inventory", False)):
            raise SystemExit("--inventory_evidence needs --track --inventory: the pictures belong to the inventory's signs")
        if getattr(args, "inventory_evidence", None) is None:
            raise SystemExit("--inventory_evidence_scale needs --inventory_evidence E")
        E, S = args.inventory_evidence, getattr(args, "inventory_evidence_scale", None)
        if not (32 <= E <= 256 and E % 16 == 0):
            raise SystemExit(f"--inventory_evidence {E} is no multiple of 16 in 32..256")
        if S is not None and not 1.0 <= S <= 16.0:
            raise SystemExit(f"--inventory_evidence_scale {S} outside 1..16")
    if getattr(args, "track", False):   # tracking needs the frames of ONE sequence, all of them, in order, in one process
        if not args.raw_frames:
            raise SystemExit("--track needs --raw_frames: the frames of a raw file are a sequence, the images of --input are not")
        if args.num_samples:
            raise SystemExit("--track and --num_samples exclude each other: a sample of the frames is not a sequence")
        if args.gpus > 1:
            raise SystemExit(f"--track and --gpus {args.gpus} exclude each other: the shards of a sequence cannot be tracked apart")
    if args.raw_frames and not args.frame_size:
        raise SystemExit("--raw_frames needs --frame_size WxH")
    if args.raw_frames:   # a malformed size or a trailing partial frame is reported before any model is loaded
        fw, fh = parse_frame_size(args.frame_size)
        read_raw_frames(args.raw_frames, fw, fh, args.pixel_format)
    if args.pixel_format != "bgr" and not args.raw_frames:
        raise SystemExit(f"--pixel_format {args.pixel_format} describes the frames of --raw_frames; images of --input are decoded to BGR")


def run_evaluation(args) -> Dict:
    """The reference's main loop (e2e.py:1090-1130) over image CHUNKS of --batch_images: per chunk one benchmark pass at
    --benchmark_conf (its wall time feeds the FPS figure) and, unless the two thresholds are equal, one evaluation pass at
    --yolo_conf whose detections feed the metric (process_image, e2e.py:953-1011).  Returns everything main() prints/writes."""
    from .backend import HybridPipeline

    from . import distributed as D

    check_frame_args(args)
    args.track = bool(getattr(args, "track", False))
    args.inventory = bool(getattr(args, "inventory", False))
    rank, local_rank, world = D.env_rank_world()
    if args.track and world > 1:   # a launcher's WORLD_SIZE shards the files as --gpus does
        raise SystemExit(f"--track runs in one process: the shards of a sequence cannot be tracked apart (WORLD_SIZE is {world})")
    if args.gpus > 1 or world > 1:
        import torch
        import torch.distributed as dist
        if world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} needs one process per GPU: launch with torch.distributed.run --nproc-per-node "
                             f"{args.gpus} (WORLD_SIZE is {world})")
        backend = os.environ.get("LITEPI_DIST_BACKEND", "nccl")   # "gloo": the CPU tests of the shard / merge logic
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29541")
            if backend == "nccl":
                torch.cuda.set_device(local_rank)
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
        args.hip_device = local_rank
        gather_device = torch.device("cuda", local_rank) if backend == "nccl" else "cpu"
    else:
        gather_device = "cpu"
    say = print if rank == 0 else (lambda *a, **k: None)

    class_names = load_class_names(args.classes)
    num_classes = len(class_names)
    if getattr(args, "detector_onnx", None):
        args.detector_param, args.detector_bin = args.detector_onnx, None
    detector_name = Path(args.detector_param).stem
    combo = f"{detector_name}+{args.clf_arch}"
    say(f"\n{'=' * 60}\nMODEL COMBINATION: {combo}\n{'=' * 60}")
    nb = max(1, args.batch_images)
    max_det = args.max_det if args.max_det > 0 else num_anchors(args.det_input_size)
    max_batch, max_rois = nb, args.max_rois
    if args.tile_overlap is not None:   # room for the views of batch_images TT100K-size frames; ROIs are still per frame
        from .backend import tile_grid
        max_batch = nb * len(tile_grid(args.det_input_size, 2048, 2048, args.tile_overlap, bool(args.tile_full_frame)))
        max_rois = max_rois if max_rois > 0 else nb * max_det
    view_kw = {}
    if getattr(args, "view_tile", None) is not None:   # likewise: the windows of batch_images TT100K-size frames
        from .backend import view_grid
        view_kw = dict(view_tile=args.view_tile, view_overlap=args.view_overlap, view_full_frame=bool(args.view_full_frame))
        max_batch = nb * len(view_grid(args.view_tile, 2048, 2048, args.view_overlap, bool(args.view_full_frame)))
        max_rois = max_rois if max_rois > 0 else nb * max_det
    elif getattr(args, "views", None) is not None:
        view_kw = dict(views=parse_views(args.views))
        max_batch = nb * len(view_kw["views"])
        max_rois = max_rois if max_rois > 0 else nb * max_det
    map_frame = None
    if getattr(args, "view_maps", None) is not None:   # the listed views, then every map, per frame
        xy, map_frame = load_view_maps(args.view_maps, args.det_input_size)
        view_kw.update(view_maps=list(xy), view_maps_frame=map_frame)
        max_batch = nb * (len(view_kw.get("views", [])) + len(xy))
        max_rois = max_rois if max_rois > 0 else nb * max_det
    if getattr(args, "focus", None) is not None:   # one whole-frame view and --focus windows per frame
        view_kw = dict(focus=args.focus, focus_config=dict(side_max=args.focus_side_max, margin=args.focus_margin,
                                                           sweep=0 if args.no_focus_sweep else 1))
        max_batch = nb * (1 + args.focus)
        max_rois = max_rois if max_rois > 0 else nb * max_det
    for name in ("view_match", "view_merge", "view_match_thr"):   # absent: the pipeline is constructed exactly as before
        if getattr(args, name, None) is not None:
            view_kw[name] = getattr(args, name)
    import contextlib
    import io
    files, raw, label_dir, (fw, fh) = list_inputs(args)
    # with --track off the pipeline is constructed and called exactly as before
    track_kw = dict(track=True, track_config=dict(iou_match=args.track_iou, max_age=args.track_max_age, min_hits=args.track_min_hits)) if args.track else {}
    if args.inventory:
        track_kw["inventory"] = dict(best=args.inventory_best)
    evidence_on = args.inventory and getattr(args, "inventory_evidence", None) is not None
    if evidence_on:   # absent: the pipeline is constructed exactly as before
        track_kw["evidence"] = dict(size=args.inventory_evidence)
        if getattr(args, "inventory_evidence_scale", None) is not None:
            track_kw["evidence"]["scale"] = args.inventory_evidence_scale
    quality_on = quality_wanted(args)
    if quality_on:   # absent: the pipeline is constructed exactly as before
        track_kw["quality"] = True
    if getattr(args, "topk", None) is not None:   # absent: the pipeline is constructed exactly as before
        track_kw["topk"] = args.topk
        if getattr(args, "track_vote", "top1") != "top1":
            track_kw["track_vote"] = args.track_vote
    bench_kw, eval_kw = (dict(track=True), dict(track=False)) if args.track else ({}, {})
    device_eval = bool(getattr(args, "device_eval", False))
    if device_eval:   # absent: the pipeline is constructed and called exactly as before
        if world > 1:
            raise SystemExit(f"--device_eval runs in one process (WORLD_SIZE is {world})")
        # the log holds every record of the evaluation pass
        track_kw["evaluate"] = dict(max_gt=args.device_eval_max_gt, max_rows=max(1, min(len(files) * max_det, 1 << 27)))
        one_pass = args.yolo_conf == args.benchmark_conf   # then the benchmark pass is the evaluation pass, as without the flag
    with contextlib.redirect_stdout(io.StringIO()) if rank != 0 else contextlib.nullcontext():   # one banner, rank 0's
        pipeline = HybridPipeline(args.detector_param, args.detector_bin, args.classifier, args.clf_arch, num_classes,
                                  args.det_input_size, args.cls_input_size, False, args.detector_threads, args.device,
                                  args.batch_size, precision=args.precision, max_batch=max_batch, max_det=max_det,
                                  device=args.hip_device, max_rois=max_rois, numerics=args.numerics,
                                  tile_overlap=args.tile_overlap, tile_full_frame=bool(args.tile_full_frame),
                                  pixel_format=args.pixel_format, csc_matrix=args.csc_matrix, **view_kw, **track_kw)
    out_dir = Path(args.output) / combo
    out_dir.mkdir(parents=True, exist_ok=True)

    say(f"\nFound {len(files)} images for processing" + (f" ({world} ranks, contiguous shards)" if world > 1 else ""))
    n_total = len(files)
    lo, hi = D.shard_range(n_total, rank, world)
    files = files[lo:hi]

    all_preds, all_gts, bench_time, names = [], [], 0.0, []
    track_rows, signs, focus_rows = [], [], []
    try:
        n_warm = args.warmup if args.warmup is not None else (10 if args.numerics == "e2e_optimize" else 0)
        if n_warm > 0:   # warmup_pipeline (e2e_optimize.py:552-570): random frame, conf 0.5
            wh, ww = 640, 640
            for v in view_kw.get("views", []):   # --views windows are frame pixels: the warm-up frame must hold them
                if v != "full":
                    wh, ww = max(wh, v[1] + v[3] + (v[1] + v[3]) % 2), max(ww, v[0] + v[2] + (v[0] + v[2]) % 2)
            if map_frame is not None:   # --view_maps: the maps belong to one frame size
                wh, ww = map_frame
            dummy = np.random.randint(0, 255, (wh * 3 // 2, ww) if args.pixel_format == "nv12" else (wh, ww, 3), dtype=np.uint8)
            for _ in range(n_warm):
                if args.track:   # the warm-up frames are not part of the sequence: they never reach the tracker
                    pipeline.run_batch([dummy], 0.5, track=False, **({"evaluate": False} if device_eval else {}))
                else:
                    pipeline.run(dummy, conf_threshold=0.5)
            say(f"Warmup complete ({n_warm} passes)")
        for i in range(0, len(files), nb):
            chunk, imgs = [], []
            for f in files[i:i + nb]:
                im = np.ascontiguousarray(raw[f.index]) if raw is not None else read_image_bgr(f)
                if im is None:
                    print(f"\nSkipping {f.name}")
                    continue
                chunk.append(f)
                imgs.append(im)
            if not imgs:
                continue
            # the tracker is fed exactly once per frame: by the benchmark pass; the evaluation pass is not tracked
            chunk_gts = None
            if device_eval:   # the labels are parsed once, in front of the pass that hands them to the evaluator
                chunk_gts = []
                for f, im in zip(chunk, imgs):
                    lp = (label_dir / f"{f.stem}.txt") if label_dir else f.parent / "labels" / f"{f.stem}.txt"
                    im_h, im_w = (fh, fw) if raw is not None else im.shape[:2]
                    chunk_gts.append(parse_yolo_label(lp, im_w, im_h))
                    check_device_eval_labels(chunk_gts[-1], args.device_eval_max_gt, lp)
            scored_kw = dict(gts=chunk_gts) if device_eval else {}
            bench = pipeline.run_batch(imgs, args.benchmark_conf, args.iou_threshold, args.min_area, **bench_kw,
                                       **(scored_kw if device_eval and one_pass else {"evaluate": False} if device_eval else {}))
            bench_time += sum(m.t_total for _, m in bench) / 1000.0
            bench_views = list(getattr(pipeline, "last_focus_views", []))
            if device_eval:
                ev = bench if one_pass else pipeline.run_batch(imgs, args.yolo_conf, args.iou_threshold, args.min_area, **eval_kw, **scored_kw)
            else:
                ev = bench if args.yolo_conf == args.benchmark_conf else pipeline.run_batch(imgs, args.yolo_conf, args.iou_threshold, args.min_area, **eval_kw)
            if getattr(args, "focus", None) is not None:   # the windows of the benchmark pass, the one the tracker follows
                for f, wins in zip(chunk, bench_views):
                    focus_rows += [(f.index, k, *w) for k, w in enumerate(wins)]
            if args.track:
                for f, (res, _) in zip(chunk, bench):
                    track_rows += [(f.index, r["track_id"], *r["bbox"], r["det_conf"], r["cls_class"], r["cls_conf"], r["track_cls"],
                                    r["track_cls_conf"], r["track_hits"], int(r["track_confirmed"]),
                                    *(("" if r[k] is None else r[k] for k in QUALITY_CSV_COLUMNS) if quality_on else ())) for r in res]
                if args.inventory:
                    signs += pipeline.drain_signs()
            for k, (f, im, (res, _)) in enumerate(zip(chunk, imgs, ev)):
                lp = (label_dir / f"{f.stem}.txt") if label_dir else f.parent / "labels" / f"{f.stem}.txt"
                im_h, im_w = (fh, fw) if raw is not None else im.shape[:2]
                all_gts.append(chunk_gts[k] if chunk_gts is not None else parse_yolo_label(lp, im_w, im_h))
                if args.save_viz:   # overlays of the evaluation pass, e2e.py:1003-1009
                    viz_dir = out_dir / "visualizations"
                    viz_dir.mkdir(parents=True, exist_ok=True)
                    if args.pixel_format == "nv12":   # the overlay is drawn on a host conversion with the device's arithmetic
                        from .pixfmt import nv12_to_bgr
                        im = nv12_to_bgr(im, args.csc_matrix)
                    visualize_prediction(im, res, all_gts[-1], class_names, viz_dir / f"vis_{f.stem}.png")
                all_preds.append([{"bbox": r["bbox"], "conf": r.get("det_conf", 0.0), "cls_class": r.get("cls_class", -1)} for r in res])
                names.append(f.name)
        if args.inventory:   # the end of the sequence: the tracks still open are signs too
            signs += pipeline.drain_signs(flush=True)
        device_metrics = pipeline.evaluation() if device_eval else None
        if device_eval and pipeline.eval_rows_dropped:
            raise SystemExit(f"--device_eval: {pipeline.eval_rows_dropped} records did not fit the evaluator's log; lower --max_det or "
                             f"raise --yolo_conf")
    finally:
        pipeline.engine.close()
    if args.track:
        import csv
        with open(out_dir / "tracks.csv", "w", newline="") as fcsv:
            w = csv.writer(fcsv)
            w.writerow(TRACKS_CSV_COLUMNS + (QUALITY_CSV_COLUMNS if quality_on else ()))
            w.writerows(track_rows)
        confirmed = {r[1] for r in track_rows if r[len(TRACKS_CSV_COLUMNS) - 1] and r[1] > 0}
        say(f"Tracking: {len(confirmed)} confirmed tracks over {len(files)} frames ({len(track_rows)} detections) -> {out_dir / 'tracks.csv'}")
    if getattr(args, "focus", None) is not None:
        import csv
        with open(out_dir / "focus.csv", "w", newline="") as fcsv:
            w = csv.writer(fcsv)
            w.writerow(("frame", "slot", "x", "y", "w", "h"))
            w.writerows(focus_rows)
        used = sum(1 for r in focus_rows if r[4] > 0)
        say(f"Focus views: {used} windows in {len(focus_rows)} slots over {len(files)} frames -> {out_dir / 'focus.csv'}")
    if args.inventory:
        import csv
        from PIL import Image
        crop_dir = out_dir / "signs"
        crop_dir.mkdir(parents=True, exist_ok=True)
        with open(out_dir / "signs.csv", "w", newline="") as fcsv:
            w = csv.writer(fcsv)
            w.writerow(SIGNS_CSV_COLUMNS + (EVIDENCE_CSV_COLUMNS if evidence_on else ()))
            for s in signs:
                name = ""
                if s["crop"] is not None:
                    name = f"signs/sign_{s['stream']}_{s['track_id']}.png"
                    Image.fromarray(s["crop"], "RGB").save(out_dir / name)
                win = ()
                if evidence_on:
                    win = s["evidence_window"] or ("", "", "", "")
                    if s["evidence"] is not None:   # BGR, the frames' byte order -> the PNG's RGB
                        Image.fromarray(np.ascontiguousarray(s["evidence"][:, :, ::-1]), "RGB").save(
                            out_dir / f"signs/sign_{s['stream']}_{s['track_id']}_evidence.png")
                w.writerow((s["stream"], s["track_id"], s["first_frame"], s["last_frame"], s["hits"], s["cls"], s["cls_conf"], s["best_frame"],
                            *s["bbox"], s["det_class"], int(s["flushed"]), name, *win))
        say(f"Inventory: {len(signs)} signs ({sum(s['crop'] is not None for s in signs)} with a crop, {pipeline.signs_dropped} dropped) "
            f"-> {out_dir / 'signs.csv'}")
    rank_times = [bench_time]
    if world > 1:   # the one exchange of the sharded evaluation: every rank's predictions + ground truths -> rank 0
        import torch.distributed as dist
        got = D.gather_eval_shards(all_preds, all_gts, bench_time, device=gather_device)
        dist.barrier()
        if rank != 0:
            return {"rank": rank, "files": names}
        all_preds, all_gts, rank_times = got
    m = device_metrics if device_eval else evaluate_predictions(all_preds, all_gts, num_classes, args.iou_threshold)
    # one rank: the reference's figure, mean per-image benchmark time; N ranks: the sharded job takes as long as its slowest rank
    avg = max(rank_times) / len(all_preds) if all_preds else 0.0
    return {"combo": combo, "detector": detector_name, "class_names": class_names, "metrics": m, "avg_time": avg,
            "fps": 1.0 / avg if avg > 0 else 0.0, "all_preds": all_preds, "all_gts": all_gts, "files": names, "max_det": max_det,
            "rank": 0, "world": world, "rank_bench_times": rank_times}


def main(argv=None) -> int:
    import pandas as pd

    args = build_parser().parse_args(argv)
    r = run_evaluation(args)
    if r.get("rank", 0) != 0:   # --gpus N: rank 0 alone scores, prints and writes
        return 0
    combo, m, class_names, fps, avg = r["combo"], r["metrics"], r["class_names"], r["fps"], r["avg_time"]
    print("\n" + "=" * 80 + f"\nEVALUATION RESULTS - {combo}\n" + "=" * 80)
    print(f"\nPerformance Metrics (at conf={args.benchmark_conf}):\n  Avg Inference Time: {avg * 1000:.2f} ms\n  Real FPS:           {fps:.2f} FPS")
    print(f"\nAccuracy Metrics (at conf={args.yolo_conf}):")
    print(f"{'Class':<20} {'Precision':>10} {'Recall':>10} {'F1':>10} {'TP':>6} {'FP':>6} {'FN':>6}\n" + "-" * 80)
    valid = m["classes_present"]
    for c, name in enumerate(class_names):
        if valid[c]:
            print(f"{name:<20} {m['precision'][c]:>10.3f} {m['recall'][c]:>10.3f} {m['f1'][c]:>10.3f} "
                  f"{int(m['tp'][c]):>6} {int(m['fp'][c]):>6} {int(m['fn'][c]):>6}")
    mean = lambda k: float(np.mean(m[k][valid])) if valid.any() else 0.0  # noqa: E731
    print("-" * 80 + f"\n{'MEAN':<20} {mean('precision'):>10.3f} {mean('recall'):>10.3f} {mean('f1'):>10.3f}")
    print(f"{'mAP@0.5':<20} {m['mAP50']:>10.3f}\n{'mAP@0.5:0.95':<20} {m['mAP50_95']:>10.3f}")
    row = pd.DataFrame([{"model_combination": combo, "detector": r["detector"], "classifier": args.clf_arch,
                         "num_test_images": len(r["all_preds"]), "mean_precision": mean("precision"), "mean_recall": mean("recall"),
                         "mean_f1": mean("f1"), "fps": fps, "mAP50": m["mAP50"], "mAP50-95": m["mAP50_95"]}])
    summary = Path(args.output) / "comparison_summary.csv"
    if summary.exists():
        row = pd.concat([pd.read_csv(summary), row], ignore_index=True)
    row.to_csv(summary, index=False)
    print(f"Updated comparison summary at {summary}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
