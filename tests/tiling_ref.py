"""CPU oracle of tiled inference (test infrastructure only; include/litepi.h "tiled inference" states the semantics).

Built from the existing oracle functions: views are NumPy slices of the frame (crops) or ``postprocess_ref.letterbox`` (the
whole frame), every view goes through ``ncnn_ref.run_graph``, the per-view filter + transform restates
``postprocess_ref.postprocess`` up to its clip with the view's geometry, the candidates of all views are concatenated
view-major and go through ``postprocess_ref.nms`` per class: its stable descending order over the concatenation is the
library's tie rule (higher (view, anchor) first).
"""
from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import ncnn_ref, postprocess_ref as P


def tile_axis(L: int, S: int, overlap: int) -> List[int]:
    if L <= S:
        return [0]
    step = S - overlap
    n = 1 + -(-(L - S) // step)
    return [min(k * step, L - S) for k in range(n)]


def tile_grid(S: int, H: int, W: int, overlap: int = 128, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
    """(x, y, w, h) windows; (-1, -1, W, H) is the letterboxed whole frame."""
    if not 0 <= overlap < S:
        raise ValueError(f"overlap {overlap} outside 0..{S - 1}")
    xs, ys = tile_axis(W, S, overlap), tile_axis(H, S, overlap)
    views = []
    if len(xs) * len(ys) == 1 or full_frame:
        views.append((-1, -1, W, H))
    if len(xs) * len(ys) > 1:
        views += [(x, y, S, S) for y in ys for x in xs]
    return views


def make_views(img: np.ndarray, S: int, overlap: int = 128, full_frame: bool = True):
    """[(view uint8 [S,S,3], ratio, (pad_w, pad_h))] in view order."""
    H, W = img.shape[:2]
    out = []
    for x, y, _, _ in tile_grid(S, H, W, overlap, full_frame):
        if x < 0:
            lb, r, pad = P.letterbox(img, S)
            out.append((lb, r, pad))
        else:
            v = np.full((S, S, 3), 114, np.uint8)
            crop = img[y:y + S, x:x + S]
            v[:crop.shape[0], :crop.shape[1]] = crop
            out.append((v, 1.0, (-float(x), -float(y))))
    return out


def view_candidates(out0: np.ndarray, orig_shape, ratio, pad, conf: float):
    """postprocess_ref.postprocess up to the clip: (xyxy float32 [n,4], scores, class ids, anchors) in anchor order."""
    ratio, pad, conf = float(ratio), (float(pad[0]), float(pad[1])), float(conf)
    pred = np.asarray(out0)
    boxes, scores = pred[:4].T, pred[4:].T
    cs, ci = scores.max(axis=1), scores.argmax(axis=1)
    mask = cs > conf
    anchors = np.nonzero(mask)[0]
    boxes, cs, ci = boxes[mask], cs[mask], ci[mask]
    xc, yc, bw, bh = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    xyxy = np.stack([xc - bw / 2, yc - bh / 2, xc + bw / 2, yc + bh / 2], axis=1)
    xyxy[:, [0, 2]] -= pad[0]
    xyxy[:, [1, 3]] -= pad[1]
    xyxy /= ratio
    xyxy[:, [0, 2]] = np.clip(xyxy[:, [0, 2]], 0, orig_shape[1])
    xyxy[:, [1, 3]] = np.clip(xyxy[:, [1, 3]], 0, orig_shape[0])
    return xyxy.astype(np.float32), cs.astype(np.float32), ci.astype(np.int64), anchors.astype(np.int64)


def merge(boxes, scores, classes, views, anchors, iou: float, max_det: Optional[int] = None):
    """One per-class greedy NMS over a frame's candidates given view-major (views ascending, anchors ascending within a view).
    Returns the indices of the kept candidates in output order (class ascending, score descending; ties: higher (view,
    anchor) first); with max_det, the max_det best (score, view, anchor) over all classes stay."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores, classes = np.asarray(scores, np.float32), np.asarray(classes)
    views, anchors = np.asarray(views, np.int64), np.asarray(anchors, np.int64)
    order = np.lexsort((anchors, views))
    assert np.array_equal(order, np.arange(len(order))), "candidates must come view-major, anchors ascending"
    idx: List[int] = []
    for c in np.unique(classes):
        m = np.nonzero(classes == c)[0]
        idx.extend(m[P.nms(boxes[m], scores[m], iou)].tolist())
    if max_det is not None and len(idx) > max_det:
        key = sorted(idx, key=lambda i: (scores[i].item(), views[i], anchors[i]), reverse=True)[:max_det]
        keep = set(key)
        idx = [i for i in idx if i in keep]
    return np.array(idx, np.int64)


class CpuTiledPipeline:
    """CpuPipeline.run (oracle/pipeline_ref.py) with the frame seen through its views."""

    def __init__(self, det_layers, cls_model=None, input_size: int = 640, cls_input: int = 64):
        self.layers, self.cls, self.S, self.cls_input = det_layers, cls_model, input_size, cls_input

    @torch.no_grad()
    def candidates(self, img: np.ndarray, conf: float, overlap: int, full_frame: bool):
        """every view's filtered candidates in frame coordinates, view-major: (boxes, scores, classes, views, anchors)"""
        bs, ss, cs, vs, an = [], [], [], [], []
        for k, (v, r, pad) in enumerate(make_views(img, self.S, overlap, full_frame)):
            x, _, _ = P.preprocess(v, self.S)   # an S x S view: the letterbox is the identity
            out0 = ncnn_ref.run_graph(self.layers, torch.from_numpy(x))["out0"].numpy()[0]
            b, s, c, a = view_candidates(out0, img.shape[:2], r, pad, conf)
            bs.append(b); ss.append(s); cs.append(c); an.append(a); vs.append(np.full(len(a), k, np.int64))
        return (np.concatenate(bs).reshape(-1, 4), np.concatenate(ss), np.concatenate(cs), np.concatenate(vs), np.concatenate(an))

    def detect(self, img, conf, iou, overlap=128, full_frame=True, max_det=None):
        b, s, c, v, a = self.candidates(img, conf, overlap, full_frame)
        k = merge(b, s, c, v, a, iou, max_det)
        return b[k], s[k], c[k]

    def run(self, img, conf=0.5, iou=0.45, min_area=100, overlap=128, full_frame=True):
        from oracle import shufflenet_ref
        boxes, scores, det_cls = self.detect(img, conf, iou, overlap, full_frame)
        num = len(boxes)
        h, w = img.shape[:2]
        rects, valid = P.roi_rects(boxes, h, w, min_area)
        rois = [img[y1:y2, x1:x2] for x1, y1, x2, y2 in rects]
        ids = shufflenet_ref.predict_batch(self.cls, rois, self.cls_input)[0] if (rois and self.cls is not None) else []
        boxes, scores, det_cls = boxes[valid], scores[valid], det_cls[valid]
        res = [{"bbox": tuple(boxes[i].astype(int)), "det_class": int(det_cls[i]), "det_conf": float(scores[i]),
                "cls_class": int(ids[i]) if i < len(ids) else -1} for i in range(len(boxes))]
        return res, num
